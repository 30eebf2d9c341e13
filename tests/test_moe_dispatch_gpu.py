"""Fused MoE token path on the GPU (csrc/kernels/moe_route.hip,
csrc/kernels/moe_dispatch.hip; ops/moe.py): expert sort, dispatch, combine
and the top-k router against torch / fp64 references, and the MoELayer on
them against an fp32 per-expert reference with the routing frozen."""

import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dlrover_wuqiong_amd._native import kernels

    kernels(required=True)


# ------------------------------------------------------------------ sort

# The sort kernels give every block a chunk of 2048 assignments (4 waves x
# 512); the largest case below, n = 3000 * 8 = 24000, spans 12 chunks.
SORT_CHUNK = 2048


def _sort_case(T, k, nb):
    g = torch.Generator().manual_seed(T * 31 + nb)
    idx = torch.randint(0, nb, (T, k), generator=g)
    if (T, k, nb) == (1000, 3, 5):
        idx[idx == 2] = 3  # bucket 2 empty
    if (T, k, nb) == (2048, 1, 16):
        idx.fill_(11)  # every assignment in one bucket
    if nb == 257:
        assert (idx == 256).any()  # sentinel entries
    return idx


@pytest.mark.parametrize("T,k,nb", [(1, 1, 1), (77, 2, 8), (1000, 3, 5), (2048, 1, 16), (4099, 2, 64),
                                    (3000, 8, 257)])
def test_sort_bit_exact(T, k, nb):
    from dlrover_wuqiong_amd.ops import _hip
    from dlrover_wuqiong_amd.ops.moe import sort_by_expert

    assert _hip.lib().dw_moe_sort_chunk_size() == SORT_CHUNK
    idx = _sort_case(T, k, nb).cuda()
    order, pos, counts = sort_by_expert(idx, nb)
    flat = idx.reshape(-1)
    ref = torch.argsort(flat, stable=True)
    assert order.dtype == torch.int32 and pos.dtype == torch.int32 and counts.dtype == torch.int64
    assert torch.equal(order.long(), ref)
    inv = torch.empty_like(ref).scatter_(0, ref, torch.arange(T * k, device="cuda"))
    assert torch.equal(pos.long(), inv)
    assert torch.equal(counts, torch.bincount(flat, minlength=nb))


def test_sort_largest_case_spans_chunks():
    assert 3000 * 8 > 2 * SORT_CHUNK


# ------------------------------------------------------------------ dispatch / combine

T_, K_, E_ = 300, 3, 8


@pytest.fixture(scope="module")
def routing():
    """One assignment with sentinel entries, sorted once (torch) and shared."""
    if not torch.cuda.is_available():  # module scope: set up before the per-test skip above
        pytest.skip("no GPU")
    g = torch.Generator().manual_seed(7)
    idx = torch.stack([torch.randperm(E_, generator=g)[:K_] for _ in range(T_)])
    idx = torch.where(torch.rand(T_, K_, generator=g) < 0.25, torch.full_like(idx, E_), idx).cuda()
    flat = idx.reshape(-1)
    order = torch.argsort(flat, stable=True)
    pos = torch.empty_like(order).scatter_(0, order, torch.arange(T_ * K_, device="cuda"))
    counts = torch.bincount(flat, minlength=E_ + 1)
    valid = flat[order] < E_
    assert 0 < int(counts[E_]) < T_ * K_
    return dict(idx=idx, order=order, pos=pos, counts=counts, valid=valid,
                order32=order.int(), pos32=pos.int())


def _close_one_ulp(got, ref32, k, scale_max):
    """One bf16 ulp of the fp32 reference: rtol 2^-7, atol k 2^-20 max|.|."""
    err = (got.float() - ref32).abs()
    bound = 2.0 ** -7 * ref32.abs() + k * 2.0 ** -20 * scale_max
    print("max err", err.max().item(), "max bound slack", (err - bound).max().item())
    return bool((err <= bound).all())


@pytest.mark.parametrize("H", [8, 264, 4096])
def test_dispatch_forward_backward(routing, H):
    from dlrover_wuqiong_amd.ops.moe import moe_dispatch

    r = routing
    g = torch.Generator().manual_seed(H)
    x = torch.randn(T_, H, generator=g).cuda().bfloat16().requires_grad_(True)
    xs = moe_dispatch(x, r["order32"], r["pos32"], K_, r["counts"], E_)
    ref = x.detach().index_select(0, r["order"] // K_)
    ref = torch.where(r["valid"].unsqueeze(-1), ref, ref.new_zeros(()))
    assert torch.equal(xs, ref)
    # backward: the grouped gradient rows past n_valid hold NaN and must not be read
    gy = torch.randn(T_ * K_, H, generator=g).cuda().bfloat16()
    gy = torch.where(r["valid"].unsqueeze(-1), gy, gy.new_full((), float("nan")))
    (dx1,) = torch.autograd.grad(xs, x, gy, retain_graph=True)
    (dx2,) = torch.autograd.grad(xs, x, gy)
    assert torch.equal(dx1, dx2)
    gz = torch.where(r["valid"].unsqueeze(-1), gy, gy.new_zeros(())).float()
    ref32 = torch.zeros(T_ * K_, H, device="cuda").index_copy(0, r["order"], gz).view(T_, K_, H).sum(1)
    assert torch.isfinite(dx1).all()
    assert _close_one_ulp(dx1, ref32, K_, gz.abs().max().item())


@pytest.mark.parametrize("H", [8, 264, 4096])
def test_combine_forward_backward(routing, H):
    from dlrover_wuqiong_amd.ops.moe import moe_combine

    r = routing
    n = T_ * K_
    g = torch.Generator().manual_seed(100 + H)
    valid = r["valid"].unsqueeze(-1)
    y0 = torch.randn(n, H, generator=g).cuda().bfloat16()
    y = torch.where(valid, y0, y0.new_full((), float("nan"))).requires_grad_(True)  # sentinel rows: NaN
    w = (torch.rand(T_, K_, generator=g).cuda() * (r["idx"] < E_)).requires_grad_(True)
    out = moe_combine(y, w, r["order32"], r["pos32"], K_, r["counts"], E_)
    assert torch.isfinite(out).all()
    yz = torch.where(valid, y0, y0.new_zeros(())).float()
    buf = torch.zeros(n, H, device="cuda").index_copy(0, r["order"], yz).view(T_, K_, H)
    ref32 = (buf * w.detach().unsqueeze(-1)).sum(1)
    assert _close_one_ulp(out, ref32, K_, (buf * w.detach().unsqueeze(-1)).abs().max().item())

    go = torch.randn(T_, H, generator=g).cuda().bfloat16()
    dy, dw = torch.autograd.grad(out, (y, w), go)
    # dy: w * dout in fp32, one rounding to bf16; zero in the sentinel rows
    wf = w.detach().reshape(-1)[r["order"]].unsqueeze(-1)
    dy_ref = (wf * go.float().index_select(0, r["order"] // K_)).bfloat16()
    dy_ref = torch.where(valid, dy_ref, dy_ref.new_zeros(()))
    assert torch.equal(dy, dy_ref)
    # dw: fp32 sum of H products against fp64, bound H 2^-23 sum_h |y dout|
    prod = buf.double() * go.double().unsqueeze(1)  # [T, k, H]
    dw_ref = prod.sum(-1)
    bound = H * 2.0 ** -23 * prod.abs().sum(-1)
    err = (dw.double() - dw_ref).abs()
    print("dw max err", err.max().item(), "max bound", bound.max().item())
    assert bool((err <= bound).all())
    dropped = (r["idx"] == E_)
    assert torch.equal(dw[dropped], torch.zeros_like(dw[dropped]))


# ------------------------------------------------------------------ router


def _tie_free_logits(T, E, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.stack([(torch.randperm(E, generator=g).float() - E / 2) / 32 for _ in range(T)])


def _route_ref(logits64, k, norm, a, c):
    E = logits64.shape[-1]
    probs = logits64.softmax(-1)
    w, idx = probs.topk(k, dim=-1)
    if norm:
        w = w / w.sum(-1, keepdim=True)
    counts = torch.bincount(idx.reshape(-1), minlength=E)
    frac = counts.double() / idx.numel()
    lse = torch.logsumexp(logits64, -1)
    loss = E * (frac * probs.mean(0)).sum() * a + lse.square().mean() * c
    return w, idx, lse, loss, counts


ROUTE_EK = [(E, k) for E in (4, 8, 60, 64, 160, 256) for k in (1, 2, 6, 8) if k <= E] + [(4, 4)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("E,k", ROUTE_EK)
def test_router(E, k, dtype):
    from dlrover_wuqiong_amd.ops.moe import route_forward, topk_route

    a, c = 1e-2, 1e-3
    for T in (1, 300):
        base = _tie_free_logits(T, E, seed=E * 10 + k)
        assert torch.equal(base.to(dtype).float(), base)  # exact in bf16
        for norm in (True, False):
            lg = base.to(dtype).cuda().requires_grad_(True)
            l64 = base.double().cuda().requires_grad_(True)
            w_r, idx_r, lse_r, loss_r, counts_r = _route_ref(l64, k, norm, a, c)
            raw = route_forward(lg.detach(), k, norm, a, c)
            w, idx, loss, counts = topk_route(lg, k, norm, a, c)
            assert w.dtype == torch.float32 and idx.dtype == torch.int64 and counts.dtype == torch.int64
            assert torch.equal(idx, idx_r), (T, norm)
            assert torch.equal(counts, counts_r)
            torch.testing.assert_close(w.double(), w_r.detach(), rtol=1e-5, atol=0)
            torch.testing.assert_close(raw["lse"].double(), lse_r.detach(), rtol=1e-5, atol=0)
            torch.testing.assert_close(loss.double(), loss_r.detach(), rtol=1e-5, atol=0)
            gw = torch.randn(T, k, generator=torch.Generator().manual_seed(T + k)).cuda()
            ((w * gw).sum() + 1.7 * loss).backward()
            ((w_r * gw.double()).sum() + 1.7 * loss_r).backward()
            assert lg.grad.dtype == dtype
            ref = l64.grad
            err = (lg.grad.double() - ref).abs()
            bound = 1e-4 * ref.abs().max()
            if dtype == torch.bfloat16:
                bound = bound + 2.0 ** -8 * ref.abs()
            print(E, k, T, norm, "dl max err", err.max().item(), "max|dl|", ref.abs().max().item())
            assert bool((err <= bound).all()), (T, norm)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("E,k", [(8, 2), (160, 8), (4, 4)])
def test_router_all_equal_row_takes_lowest_indices(E, k, dtype):
    from dlrover_wuqiong_amd.ops.moe import topk_route

    lg = _tie_free_logits(3, E, seed=1).to(dtype)
    lg[1] = 0.25  # one all-equal row
    w, idx, _, _ = topk_route(lg.cuda(), k)
    assert torch.equal(idx[1].cpu(), torch.arange(k))
    torch.testing.assert_close(w[1].cpu(), torch.full((k,), 1.0 / k), rtol=1e-5, atol=0)


# ------------------------------------------------------------------ layer


@pytest.mark.parametrize("capacity_factor", [0.0, 0.5])
def test_moe_layer_fused_vs_fp32_frozen_routing(capacity_factor):
    """bf16 MoELayer on the fused token path vs an fp32 per-expert reference
    that takes the layer's own expert choice (routing is tested above), so
    every token is compared; bf16 MoE tolerance 3e-2 as in test_moe_gpu."""
    from dlrover_wuqiong_amd.parallel.moe import MoELayer, capacity_mask

    torch.manual_seed(0)
    T, H, Fd, E, k = 1000, 256, 512, 8, 2
    m = MoELayer(H, Fd, num_experts=E, top_k=k, capacity_factor=capacity_factor, fused_dispatch=True)
    m = m.cuda().bfloat16()
    xg = torch.randn(T, H).cuda().bfloat16().requires_grad_(True)
    go = torch.randn(T, H).cuda().bfloat16()
    with torch.no_grad():
        _w, idx, _ = m.gate(xg)
    y = m(xg)
    ((y.float() * go.float()).sum() + m.aux_loss).backward()

    # fp32 reference on the same (bf16-rounded) values, index set frozen to idx
    x = xg.detach().float().requires_grad_(True)
    wg = m.gate.wg.weight.detach().float().requires_grad_(True)
    w1, w2, w3 = (p.detach().float() for p in (m.experts.w1, m.experts.w2, m.experts.w3))
    logits = x @ wg.t()
    probs = logits.softmax(-1)
    w = probs.gather(-1, idx)
    w = w / w.sum(-1, keepdim=True)
    frac = torch.bincount(idx.reshape(-1), minlength=E).float() / idx.numel()
    aux = E * (frac * probs.mean(0)).sum() * m.gate.aux_loss_coef + \
        torch.logsumexp(logits, -1).square().mean() * m.gate.z_loss_coef
    if capacity_factor > 0:
        keep = capacity_mask(idx, E, max(1, math.ceil(capacity_factor * T * k / E)))
        assert 0 < int((~keep).sum())
        w = w * keep
    yr = torch.zeros(T, H, device="cuda")
    for e in range(E):
        h = F.silu(x @ w1[e].t()) * (x @ w3[e].t())
        ye = h @ w2[e].t()
        yr = yr + ye * (w * (idx == e)).sum(-1, keepdim=True)
    ((yr * go.float()).sum() + aux).backward()

    def rel(a, b):
        return ((a.float() - b).norm() / b.norm()).item()

    figs = dict(out=rel(y, yr.detach()), dx=rel(xg.grad, x.grad), dwg=rel(m.gate.wg.weight.grad, wg.grad),
                aux=abs(m.aux_loss.item() - aux.item()) / abs(aux.item()))
    print(figs)
    assert figs["out"] < 3e-2, figs
    assert figs["dx"] < 3e-2, figs
    assert figs["dwg"] < 3e-2, figs
