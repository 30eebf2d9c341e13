"""Fused SwiGLU expert projection on the grouped GEMM (dual-weight NT forward
with the SwiGLU epilogue, dual-weight NN dgrad) vs the existing grouped
kernels (bitwise where the reduction order is shared) and the fp32
per-expert reference, and the MoE layer on it."""

import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"

# counts, H, F: the smallest shapes that reach every edge of the kernels
CASES = [
    # empty first / middle / last groups, 1-row and 128 +- 1 row blocks, a partial K iteration,
    # partial column tiles in both halves, dgrad halves not a multiple of 64
    ([0, 1, 127, 129, 0, 200, 0], 72, 72),
    ([5], 64, 64),                   # one expert, one tile, exactly one K iteration
    ([130, 0, 300], 256, 200),       # several column tiles with a ragged last one
    ([64, 0, 0, 500, 7], 520, 384),  # ragged K, several row blocks per group
]
EXTRA = 37  # trailing rows past offs[E]


def _rel(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dlrover_wuqiong_amd._native import kernels

    kernels(required=True)


def _fused_run(x, w1, w3, offs, dh):
    from dlrover_wuqiong_amd.ops.grouped_gemm import grouped_swiglu_linear

    xl, w1l, w3l = (t.detach().clone().requires_grad_() for t in (x, w1, w3))
    h = grouped_swiglu_linear(xl, w1l, w3l, offs)
    h.backward(dh)
    return h.detach(), xl.grad, w1l.grad, w3l.grad


@functools.lru_cache(maxsize=None)
def _case(i):
    """Everything the per-case tests compare, computed once."""
    from dlrover_wuqiong_amd.ops.activation import swiglu
    from dlrover_wuqiong_amd.ops.grouped_gemm import (grouped_glu_forward, grouped_linear, grouped_swiglu_reference,
                                                      offsets_from_counts)

    counts, H, F = CASES[i]
    torch.manual_seed(i)
    E, T = len(counts), sum(counts)
    x = torch.randn(T, H, device=DEV, dtype=torch.bfloat16)
    w1 = (torch.randn(E, F, H, device=DEV) / H ** 0.5).to(torch.bfloat16)
    w3 = (torch.randn(E, F, H, device=DEV) / H ** 0.5).to(torch.bfloat16)
    dh = torch.randn(T, F, device=DEV, dtype=torch.bfloat16)
    offs = offsets_from_counts(torch.tensor(counts, device=DEV), DEV)
    r = dict(counts=counts, T=T, F=F)

    # raw forward vs the existing kernels
    r["h_raw"], r["gu"] = grouped_glu_forward(x, w1, w3, offs)
    with torch.no_grad():
        r["gu_unfused"] = torch.cat([grouped_linear(x, w1, offs), grouped_linear(x, w3, offs)], 1)
    gul = r["gu"].detach().clone().requires_grad_()
    hs = swiglu(gul)
    r["h_swiglu"] = hs.detach()
    hs.backward(dh)
    dgu = gul.grad  # dw_swiglu_bwd(dh, gu), what the fused backward feeds its GEMMs

    # fused autograd function, twice (determinism)
    r["h"], r["dx"], r["dw1"], r["dw3"] = _fused_run(x, w1, w3, offs, dh)
    r["again"] = _fused_run(x, w1, w3, offs, dh)

    # fp32 oracle
    xf, w1f, w3f = (t.float().requires_grad_() for t in (x, w1, w3))
    hf = grouped_swiglu_reference(xf, w1f, w3f, offs)
    hf.backward(dh.float())
    r["ref"] = (hf.detach(), xf.grad, w1f.grad, w3f.grad)

    # the existing TN / NN kernels on contiguous copies of the two halves of dgu
    pieces = []
    for w, half in ((w1, dgu[:, :F]), (w3, dgu[:, F:])):
        xl, wl = x.clone().requires_grad_(), w.clone().requires_grad_()
        grouped_linear(xl, wl, offs).backward(half.contiguous())
        pieces.append((xl.grad, wl.grad))
    r["dw1_tn"], r["dw3_tn"] = pieces[0][1], pieces[1][1]
    r["dx_nn_sum"] = pieces[0][0].float() + pieces[1][0].float()

    # 37 rows of NaN past the last group, in x and in dh
    nan_x = torch.full((EXTRA, H), float("nan"), device=DEV, dtype=torch.bfloat16)
    nan_h = torch.full((EXTRA, F), float("nan"), device=DEV, dtype=torch.bfloat16)
    r["trail"] = _fused_run(torch.cat([x, nan_x]), w1, w3, offs, torch.cat([dh, nan_h]))
    return r


IDS = [f"H{h}-F{f}-E{len(c)}" for c, h, f in CASES]
per_case = pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)


@per_case
def test_forward_exact(i):
    r = _case(i)
    assert r["gu"].shape == (r["T"], 2 * r["F"]) and r["h_raw"].shape == (r["T"], r["F"])
    # same fragments, same BK, same k order as the NT mode: the same bits
    assert torch.equal(r["gu"], r["gu_unfused"])
    assert torch.equal(r["h_raw"], r["h_swiglu"])
    assert torch.equal(r["h"], r["h_raw"])


@per_case
def test_fwd_bwd_vs_fp32_reference(i):
    r = _case(i)
    figs = {n: _rel(a, b) for n, a, b in zip(("h", "dx", "dw1", "dw3"), (r["h"], r["dx"], r["dw1"], r["dw3"]),
                                             r["ref"])}
    print(IDS[i], figs)
    for n, v in figs.items():
        assert v < 1e-2, (n, figs)


@per_case
def test_backward_pieces(i):
    r = _case(i)
    assert torch.equal(r["dw1"], r["dw1_tn"])
    assert torch.equal(r["dw3"], r["dw3_tn"])
    v = _rel(r["dx"], r["dx_nn_sum"])
    print(IDS[i], "dx vs fp32 sum of the two NN results:", v)
    assert v < 1e-2, v


@per_case
def test_empty_experts_zero_grad(i):
    r = _case(i)
    for e, c in enumerate(r["counts"]):
        if c == 0:
            assert r["dw1"][e].abs().max() == 0 and r["dw3"][e].abs().max() == 0


@per_case
def test_trailing_rows_never_reach_a_result(i):
    r = _case(i)
    T = r["T"]
    h, dx, dw1, dw3 = r["trail"]
    assert h.shape[0] == T + EXTRA and dx.shape[0] == T + EXTRA
    for got, want in ((h[:T], r["h"]), (dx[:T], r["dx"]), (dw1, r["dw1"]), (dw3, r["dw3"])):
        assert torch.isfinite(got.float()).all()
        assert torch.equal(got, want)


@per_case
def test_deterministic(i):
    r = _case(i)
    for a, b in zip((r["h"], r["dx"], r["dw1"], r["dw3"]), r["again"]):
        assert torch.equal(a, b)


def test_shape_limits_raise():
    from dlrover_wuqiong_amd.ops._hip import HipKernelError
    from dlrover_wuqiong_amd.ops.grouped_gemm import grouped_swiglu_linear, offsets_from_counts

    offs = offsets_from_counts([4], DEV)
    for H, F, dt in ((68, 64, torch.bfloat16), (64, 60, torch.bfloat16), (64, 64, torch.float16)):
        x = torch.zeros(4, H, device=DEV, dtype=dt)
        w = torch.zeros(1, F, H, device=DEV, dtype=dt)
        with pytest.raises(HipKernelError):
            grouped_swiglu_linear(x, w, w, offs)


def test_no_rows():
    from dlrover_wuqiong_amd.ops.grouped_gemm import grouped_swiglu_linear, offsets_from_counts

    x = torch.zeros(0, 64, device=DEV, dtype=torch.bfloat16, requires_grad=True)
    w1 = torch.randn(3, 72, 64, device=DEV).to(torch.bfloat16).requires_grad_()
    w3 = torch.randn(3, 72, 64, device=DEV).to(torch.bfloat16).requires_grad_()
    h = grouped_swiglu_linear(x, w1, w3, offsets_from_counts([0, 0, 0], DEV))
    assert h.shape == (0, 72)
    h.sum().backward()
    assert x.grad.shape == (0, 64)
    assert w1.grad.abs().max() == 0 and w3.grad.abs().max() == 0


@pytest.mark.parametrize("capacity_factor", [0.0, 1.0])
def test_moe_layer_fused_experts_matches_fp32(capacity_factor):
    from dlrover_wuqiong_amd.parallel.moe import MoELayer

    torch.manual_seed(1)
    H, F, E = 256, 512, 8
    layer = MoELayer(H, F, E, top_k=2, device=DEV, dtype=torch.bfloat16, capacity_factor=capacity_factor,
                     fused_experts=True)
    ref = MoELayer(H, F, E, top_k=2, device=DEV, dtype=torch.float32, capacity_factor=capacity_factor)
    ref.load_state_dict({k: v.float() for k, v in layer.state_dict().items()})
    x = torch.randn(4, 96, H, device=DEV, dtype=torch.bfloat16, requires_grad=True)
    xf = x.detach().float().requires_grad_()
    y = layer(x)
    yr = ref(xf)  # fp32 tensors: the per-expert PyTorch loop
    y.float().pow(2).mean().backward()
    yr.pow(2).mean().backward()
    figs = dict(out=_rel(y, yr), dx=_rel(x.grad, xf.grad), dw1=_rel(layer.experts.w1.grad, ref.experts.w1.grad),
                dw3=_rel(layer.experts.w3.grad, ref.experts.w3.grad))
    print(capacity_factor, figs)
    assert figs["out"] < 3e-2, figs
    assert figs["dx"] < 5e-2 and figs["dw1"] < 5e-2 and figs["dw3"] < 5e-2, figs


def test_fused_glu_saves_fewer_activation_bytes():
    from dlrover_wuqiong_amd.parallel.moe import grouped_mlp

    torch.manual_seed(3)
    n, H, F, E = 512, 128, 256, 4
    x = torch.randn(n, H, device=DEV, dtype=torch.bfloat16, requires_grad=True)
    w1, w3 = ((torch.randn(E, F, H, device=DEV) / H ** 0.5).to(torch.bfloat16).requires_grad_() for _ in range(2))
    w2 = (torch.randn(E, H, F, device=DEV) / F ** 0.5).to(torch.bfloat16).requires_grad_()
    counts = torch.tensor([100, 0, 300, 112], device=DEV)

    def saved_bytes(fused):
        seen = {}

        def pack(t):
            seen[(t.data_ptr(), t.numel() * t.element_size())] = t.numel() * t.element_size()
            return t

        with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
            y = grouped_mlp(x, counts, w1, w2, w3, "silu", fused_glu=fused)
        return sum(seen.values()), y

    b_unfused, y0 = saved_bytes(False)
    b_fused, y1 = saved_bytes(True)
    print("saved bytes unfused / fused:", b_unfused, b_fused)
    assert _rel(y1, y0) < 1e-2
    # unfused keeps a, silu(a), b and h [n, F]; fused keeps gu [n, 2F] and h
    assert b_fused < b_unfused
