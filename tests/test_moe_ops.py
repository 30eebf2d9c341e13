"""ops/moe.py on the CPU: the torch formulation of the fused MoE token path
(router, expert sort, dispatch, combine) against the index ops and the
``TopKGate`` math it replaces, and ``MoELayer(fused_dispatch=True)`` against
``fused_dispatch=False``."""

import pytest
import torch

from dlrover_wuqiong_amd.ops import moe_combine, moe_dispatch, sort_by_expert, topk_route


def _assignment(T, k, E, sentinel_frac=0.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    idx = torch.stack([torch.randperm(E, generator=g)[:k] for _ in range(T)])
    if sentinel_frac > 0:
        drop = torch.rand(T, k, generator=g) < sentinel_frac
        idx = torch.where(drop, torch.full_like(idx, E), idx)
    return idx


@pytest.mark.parametrize("T,k,nb", [(1, 1, 1), (77, 2, 8), (500, 3, 9)])
def test_sort_by_expert_is_stable_argsort(T, k, nb):
    g = torch.Generator().manual_seed(T)
    idx = torch.randint(0, nb, (T, k), generator=g)
    if nb > 2:
        idx[idx == 1] = 0  # an empty bucket
    order, pos, counts = sort_by_expert(idx, nb)
    flat = idx.reshape(-1)
    ref = torch.argsort(flat, stable=True)
    assert order.dtype == torch.int32 and pos.dtype == torch.int32
    assert torch.equal(order.long(), ref)
    assert torch.equal(pos.long()[ref], torch.arange(T * k))
    assert torch.equal(counts, torch.bincount(flat, minlength=nb))


@pytest.mark.parametrize("sentinel", [False, True])
def test_dispatch_combine_match_index_ops_fp64(sentinel):
    T, k, E, H = 50, 3, 6, 24
    idx = _assignment(T, k, E, 0.3 if sentinel else 0.0)
    nb = E + int(sentinel)
    order, pos, counts = sort_by_expert(idx, nb)
    flat = idx.reshape(-1)
    o = torch.argsort(flat, stable=True)
    valid = (flat[o] < E).unsqueeze(-1)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(T, H, dtype=torch.float64, generator=g, requires_grad=True)
    xr = x.detach().clone().requires_grad_(True)
    xs = moe_dispatch(x, order, pos, k, counts, E)
    ref = torch.where(valid, xr.index_select(0, o // k), xr.new_zeros(()))
    assert torch.equal(xs, ref)
    gy = torch.randn(T * k, H, dtype=torch.float64, generator=g)
    xs.backward(gy)
    ref.backward(gy)
    assert torch.allclose(x.grad, xr.grad, rtol=1e-14, atol=1e-14)

    y = torch.randn(T * k, H, dtype=torch.float64, generator=g)
    w = torch.rand(T, k, dtype=torch.float64, generator=g) * (idx < E)
    y_nan = torch.where(valid, y, y.new_full((), float("nan")))  # sentinel rows must not be read
    y1 = y_nan.clone().requires_grad_(True)
    w1 = w.clone().requires_grad_(True)
    out = moe_combine(y1, w1, order, pos, k, counts, E)
    y2 = y.clone().requires_grad_(True)
    w2 = w.clone().requires_grad_(True)
    buf = torch.zeros(T * k, H, dtype=torch.float64).index_copy(0, o, torch.where(valid, y2, y2.new_zeros(())))
    ref = (buf.view(T, k, H) * w2.unsqueeze(-1)).sum(1)
    assert torch.isfinite(out).all()
    assert torch.allclose(out, ref, rtol=1e-14, atol=1e-14)
    go = torch.randn(T, H, dtype=torch.float64, generator=g)
    out.backward(go)
    ref.backward(go)
    assert torch.allclose(y1.grad, y2.grad, rtol=1e-14, atol=1e-14)
    assert torch.allclose(w1.grad, w2.grad, rtol=1e-13, atol=1e-13)


def test_combine_takes_short_y():
    """An expert-parallel y ends at n_valid: the sentinel rows are not there at all."""
    T, k, E, H = 40, 2, 4, 8
    idx = _assignment(T, k, E, 0.4, seed=3)
    order, pos, counts = sort_by_expert(idx, E + 1)
    n_valid = int(counts[:E].sum())
    y = torch.randn(T * k, H, dtype=torch.float64)
    w = torch.rand(T, k, dtype=torch.float64)
    full = moe_combine(y, w, order, pos, k, counts, E)
    short = moe_combine(y[:n_valid], w, order, pos, k, counts, E)
    assert torch.equal(full, short)


@pytest.mark.parametrize("norm_topk", [True, False])
def test_topk_route_matches_topk_gate_math(norm_topk):
    from dlrover_wuqiong_amd.parallel.moe import TopKGate

    torch.manual_seed(0)
    T, H, E, k = 64, 32, 8, 2
    gate = TopKGate(H, E, k, norm_topk=norm_topk)
    x = torch.randn(T, H)
    logits = gate.wg(x).detach()
    # today's math, written out
    l0 = logits.clone().requires_grad_(True)
    probs = l0.softmax(-1)
    w0, i0 = probs.topk(k, dim=-1)
    if norm_topk:
        w0 = w0 / w0.sum(-1, keepdim=True)
    frac = torch.bincount(i0.reshape(-1), minlength=E).float() / i0.numel()
    loss0 = E * (frac * probs.mean(0)).sum() * gate.aux_loss_coef + \
        torch.logsumexp(l0, -1).square().mean() * gate.z_loss_coef
    l1 = logits.clone().requires_grad_(True)
    w1, i1, loss1, counts = topk_route(l1, k, norm_topk, gate.aux_loss_coef, gate.z_loss_coef)
    assert torch.equal(i1, i0)
    assert torch.equal(counts, torch.bincount(i0.reshape(-1), minlength=E))
    assert torch.allclose(w1, w0, rtol=1e-6, atol=0)
    assert torch.allclose(loss1, loss0, rtol=1e-6, atol=0)
    gw = torch.randn(T, k)
    ((w0 * gw).sum() + 3.0 * loss0).backward()
    ((w1 * gw).sum() + 3.0 * loss1).backward()
    assert torch.allclose(l1.grad, l0.grad, rtol=1e-5, atol=1e-7)
    # and the module itself returns the same triple
    wm, im, lm = gate(x)
    assert torch.equal(im, i0) and torch.allclose(wm, w0, rtol=1e-6) and torch.allclose(lm, loss0, rtol=1e-6)


def test_topk_route_tie_rule_lowest_index():
    w, idx, _, counts = topk_route(torch.zeros(3, 10), 4)
    assert torch.equal(idx, torch.arange(4).expand(3, 4))
    assert torch.equal(counts, torch.tensor([3, 3, 3, 3, 0, 0, 0, 0, 0, 0]))
    assert torch.allclose(w, torch.full((3, 4), 0.25))


@pytest.mark.parametrize("capacity_factor", [0.0, 0.5])
def test_moe_layer_fused_equals_unfused_cpu(capacity_factor):
    from dlrover_wuqiong_amd.parallel.moe import MoELayer

    torch.manual_seed(0)
    a = MoELayer(32, 64, num_experts=4, top_k=2, capacity_factor=capacity_factor, fused_dispatch=False)
    b = MoELayer(32, 64, num_experts=4, top_k=2, capacity_factor=capacity_factor, fused_dispatch=True)
    b.load_state_dict(a.state_dict())
    x = torch.randn(3, 20, 32)
    xa = x.clone().requires_grad_(True)
    xb = x.clone().requires_grad_(True)
    ya, yb = a(xa), b(xb)
    assert ya.shape == yb.shape == x.shape
    assert torch.allclose(ya, yb, rtol=1e-5, atol=1e-6)
    (ya.square().sum() + a.aux_loss).backward()
    (yb.square().sum() + b.aux_loss).backward()
    assert torch.allclose(xa.grad, xb.grad, rtol=1e-4, atol=1e-5)
    for (n, pa), (_, pb) in zip(a.named_parameters(), b.named_parameters()):
        assert torch.allclose(pa.grad, pb.grad, rtol=1e-4, atol=1e-5), n
