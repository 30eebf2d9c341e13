"""Weight-streaming decode GEMM on the GPU (``csrc/kernels/skinny_gemm.hip``):
exact integer data for every tile / tail / split seam, a float bound against
fp64, determinism and graph replay, the documented fallbacks, the row
quantiser, and the hybrid engine's ``rollout_weights`` modes."""

import functools

import pytest
import torch

from conftest import gpu_available
from dlrover_wuqiong_amd.atorch.rl.hybrid_engine import HybridEngine
from dlrover_wuqiong_amd.models.llama import Llama, LlamaConfig
from dlrover_wuqiong_amd.ops import skinny_gemm
from dlrover_wuqiong_amd.ops.skinny_gemm import quantize_rows_e4m3, skinny_linear, skinny_linear_ref

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a GPU")]

# a single tile; N not a multiple of 16; M across each 16-row boundary; K % 32 == 16 (688: llama-tiny's
# down_proj); 33 k-steps (not divisible by the split); Llama-3's longest K
SHAPES = [(1, 16, 32), (5, 40, 96), (17, 48, 256), (4, 256, 688), (16, 64, 1056), (33, 100, 2080), (64, 33, 512),
          (8, 272, 14336)]
FORMS = ["bf16", "fp8"]
SPLITS = [0, 1, 2, 3]


def _gen(shape):
    return torch.Generator(device="cuda").manual_seed(1000 * shape[0] + shape[1] + shape[2])


@functools.lru_cache(maxsize=None)
def _exact_case(shape):
    """Integer data: every partial sum is an integer below 2^24, so the fp32
    result is exact in any summation order."""
    M, N, K = shape
    g = _gen(shape)
    x = torch.randint(-2, 3, (M, K), device="cuda", generator=g).to(torch.bfloat16)
    w = torch.randint(-3, 4, (N, K), device="cuda", generator=g).to(torch.bfloat16)
    scale = torch.exp2(torch.randint(-3, 3, (N,), device="cuda", generator=g).float())
    ref64 = x.double() @ w.double().T
    assert float((x.double().abs() @ w.double().abs().T).max()) < 2 ** 24
    return x, w, w.to(torch.float8_e4m3fn), scale, ref64


@pytest.mark.parametrize("splits", SPLITS)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_exact_integer_data(shape, form, splits):
    x, w, codes, scale, ref64 = _exact_case(shape)
    if form == "fp8":
        assert torch.equal(codes.float(), w.float())
        y = skinny_linear(x, codes, scale, splits=splits)
        want = (ref64.float() * scale).to(torch.bfloat16)
    else:
        y = skinny_linear(x, w, splits=splits)
        want = ref64.float().to(torch.bfloat16)
    assert y.dtype == torch.bfloat16 and y.shape == want.shape
    bad = (y != want).nonzero()
    assert bad.numel() == 0, (bad[:8].tolist(), y[tuple(bad[0])].item(), want[tuple(bad[0])].item())


@functools.lru_cache(maxsize=None)
def _float_case(shape):
    M, N, K = shape
    g = _gen(shape)
    x = torch.randn(M, K, device="cuda", generator=g).to(torch.bfloat16)
    w = torch.randn(N, K, device="cuda", generator=g)
    wb = w.to(torch.bfloat16)
    # quantised with torch, so this test does not depend on the quantiser kernel
    scale = w.abs().amax(1) / 448
    codes = (w / scale[:, None]).clamp(-448, 448).to(torch.float8_e4m3fn)
    out = {}
    for form, wt, sc in (("bf16", wb, None), ("fp8", codes, scale)):
        s64 = torch.ones(N, device="cuda", dtype=torch.float64) if sc is None else sc.double()
        ref = (x.double() @ wt.double().T) * s64
        A = (x.double().abs() @ wt.double().abs().T) * s64
        out[form] = (wt, sc, ref, A)
    return x, out


@pytest.mark.parametrize("splits", SPLITS)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_float_bound_against_fp64(shape, form, splits):
    """|y - ref| <= 2^-8 |ref| (the bf16 rounding) + K 2^-24 A (1 + 2^-8) (worst-case fp32 accumulation),
    A = scale * sum |x| |w|."""
    x, forms = _float_case(shape)
    wt, sc, ref, A = forms[form]
    y = skinny_linear(x, wt, sc, splits=splits)
    K = shape[2]
    bound = 2.0 ** -8 * ref.abs() + K * 2.0 ** -24 * A * (1 + 2.0 ** -8)
    ratio = ((y.double() - ref).abs() / bound).max()
    print(f"{shape} {form} splits={splits}: max err / bound = {float(ratio):.3f}")
    assert float(ratio) <= 1.0


@pytest.mark.parametrize("form", FORMS)
def test_deterministic_and_graph_replay(form):
    for shape, splits in (((17, 48, 256), 2), ((4, 256, 688), 0), ((8, 272, 14336), 0)):
        x, forms = _float_case(shape)
        wt, sc = forms[form][:2]
        a = skinny_linear(x, wt, sc, splits=splits)
        b = skinny_linear(x, wt, sc, splits=splits)
        assert torch.equal(a, b)
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            skinny_linear(x, wt, sc, splits=splits)   # the eager call that sizes the stream's workspace
            with torch.cuda.graph(g, stream=s):
                out = skinny_linear(x, wt, sc, splits=splits)
        torch.cuda.current_stream().wait_stream(s)
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, a)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("shape", [(65, 48, 64), (4, 32, 40)], ids=["M65", "K40"])
def test_outside_the_contract_falls_back(shape, form):
    """M > 64 and K % 16 != 0 run the torch expression and still match fp64."""
    x, forms = _float_case(shape)
    wt, sc, ref, A = forms[form]
    y = skinny_linear(x, wt, sc)
    assert y.dtype == torch.bfloat16
    assert torch.equal(y, skinny_linear_ref(x, wt, sc))
    bound = 2.0 ** -8 * ref.abs() + shape[2] * 2.0 ** -24 * A * (1 + 2.0 ** -8)
    assert ((y.double() - ref).abs() <= bound).all()
    # fp32 x is outside the contract too: fp32 math, fp32 result
    y32 = skinny_linear(x.float(), wt, sc)
    assert y32.dtype == torch.float32
    torch.testing.assert_close(y32.double(), ref, atol=1e-3, rtol=1e-3)


@pytest.mark.parametrize("form", FORMS)
def test_strided_x_matches_contiguous(form):
    shape = (33, 100, 2080)
    x, forms = _float_case(shape)
    wt, sc = forms[form][:2]
    big = torch.randn(shape[0], 2, shape[2], device="cuda").to(torch.bfloat16)
    big[:, 0] = x
    view = big[:, 0]
    assert not view.is_contiguous()
    assert torch.equal(skinny_linear(view, wt, sc), skinny_linear(x, wt, sc))
    # leading dims are flattened into M
    y3 = skinny_linear(x[:32].view(4, 8, -1), wt, sc)
    assert y3.shape == (4, 8, shape[1]) and torch.equal(y3.view(32, -1), skinny_linear(x[:32], wt, sc))


@pytest.mark.parametrize("form", FORMS)
def test_caller_owned_workspace(form):
    from dlrover_wuqiong_amd.ops import _hip

    shape = (17, 48, 256)
    x, forms = _float_case(shape)
    wt, sc = forms[form][:2]
    want = skinny_linear(x, wt, sc, splits=2)
    need = skinny_gemm.workspace_floats(17, 48, 256, form == "fp8", 2)
    assert need == 2 * 17 * 48 and skinny_gemm.workspace_floats(17, 48, 256, form == "fp8", 1) == 0
    ws = torch.full((need + 16,), float("nan"), device="cuda")
    s = torch.cuda.Stream()   # a stream the default scratch has no buffer for
    s.wait_stream(torch.cuda.current_stream())
    before = dict(_hip._SPLITK_WS)
    with torch.cuda.stream(s):
        got = skinny_linear(x, wt, sc, splits=2, workspace=ws)
    torch.cuda.current_stream().wait_stream(s)
    assert torch.equal(got, want)
    assert _hip._SPLITK_WS == before and torch.isnan(ws[need:]).all()
    with pytest.raises(ValueError, match="workspace"):
        skinny_linear(x, wt, sc, splits=2, workspace=ws[:need - 1])


@pytest.mark.parametrize("case", ["33x688", "272x4096", "zero_row", "4100x64"])
def test_quantiser_kernel(case):
    g = torch.Generator(device="cuda").manual_seed(7)
    # 4100 rows: more than the 4096 blocks of the launch, so blocks take a second row
    N, K = {"33x688": (33, 688), "272x4096": (272, 4096), "zero_row": (19, 96), "4100x64": (4100, 64)}[case]
    w = (torch.randn(N, K, device="cuda", generator=g)
         * torch.logspace(-3, 1, N, device="cuda")[:, None]).to(torch.bfloat16)
    if case == "zero_row":
        w[7] = 0
    # outputs are views into larger buffers: what lies beyond them stays untouched
    cb = torch.full((N * K + 64,), 0x5A, device="cuda", dtype=torch.uint8)
    sb = torch.full((N + 8,), -7.0, device="cuda", dtype=torch.float32)
    codes = cb[:N * K].view(N, K).view(torch.float8_e4m3fn)
    scale = sb[:N]
    got = quantize_rows_e4m3(w, out=(codes, scale))
    assert got[0].data_ptr() == codes.data_ptr() and got[1].data_ptr() == scale.data_ptr()
    assert (cb[N * K:] == 0x5A).all() and (sb[N:] == -7.0).all()
    # the reference quotients are taken on the CPU: the GPU's fp32 division in torch is not correctly rounded, and
    # a bf16 weight over a scale with a short mantissa lands on exact e4m3 ties (124 -> 128) that a quotient one
    # ulp low (123.99999 -> 120) breaks the other way
    wf = w.float()
    amax = wf.abs().amax(1)
    want = (amax.cpu() / 448).where(amax.cpu() > 0, torch.ones(N)).cuda()
    ulp = torch.nextafter(want, torch.full_like(want, float("inf"))) - want
    assert ((scale - want).abs() <= ulp).all()
    if case == "zero_row":
        assert float(scale[7]) == 1.0 and (codes[7].float() == 0).all()
    # the row's largest element maps to +-448 exactly: amax was found exactly
    assert (codes.float().abs().amax(1)[amax > 0] == 448).all()
    err = (codes.float() * scale[:, None] - wf).abs()
    assert (err <= 2.0 ** -4 * wf.abs() + 2.0 ** -10 * scale[:, None]).all()
    torch_codes = (wf.cpu() / want.cpu()[:, None]).clamp(-448, 448).to(torch.float8_e4m3fn).cuda()
    same = (codes.view(torch.uint8) == torch_codes.view(torch.uint8)).float().mean()
    assert float(same) >= 0.999, float(same)
    # a fresh pair of outputs gives the same bytes
    c2, s2 = quantize_rows_e4m3(w)
    assert torch.equal(c2.view(torch.uint8), codes.view(torch.uint8)) and torch.equal(s2, scale)


# ------------------------------------------------------------------ engine
def _model():
    torch.manual_seed(0)
    cfg = LlamaConfig.named("llama-tiny")
    with torch.device("cuda"):
        m = Llama(cfg)
    return m.to(torch.bfloat16).eval()


def _teacher_forced(eng, prompts, toks):
    eng._ensure_cache(prompts.shape[0], prompts.device, torch.bfloat16)
    eng._refresh_rollout_weights()
    out = [eng._forward(prompts, prefill=True)]
    for t in range(toks.shape[1]):
        out.append(eng._forward(toks[:, t:t + 1], prefill=False).clone())
    return torch.stack(out)


@torch.no_grad()
@pytest.mark.parametrize("mode", FORMS)
def test_engine_decode_logits_match_torch_math(mode, monkeypatch):
    m = _model()
    prompts = torch.randint(1, m.cfg.vocab_size, (4, 9), device="cuda")
    toks = torch.randint(1, m.cfg.vocab_size, (4, 6), device="cuda")
    calls = []
    real = skinny_gemm.skinny_linear
    monkeypatch.setattr(skinny_gemm, "skinny_linear", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    got = _teacher_forced(HybridEngine(m, 4, 32, use_graph=False, rollout_weights=mode), prompts, toks)
    # five GEMMs per decode step: four per layer + the head
    assert len(calls) == 6 * (4 * m.cfg.num_hidden_layers + 1)
    monkeypatch.setattr(skinny_gemm, "skinny_linear", lambda x, w, scale=None, splits=0, workspace=None: skinny_linear_ref(x, w, scale))
    want = _teacher_forced(HybridEngine(m, 4, 32, use_graph=False, rollout_weights=mode), prompts, toks)
    torch.testing.assert_close(got.float(), want.float(), atol=5e-2, rtol=5e-2)


@torch.no_grad()
@pytest.mark.parametrize("fused", [False, True], ids=["unfused_kv", "fused_kv"])
@pytest.mark.parametrize("mode", FORMS)
def test_engine_graph_decode_equals_eager(mode, fused):
    m = _model()
    prompts = torch.randint(1, m.cfg.vocab_size, (4, 12), device="cuda")
    lens = torch.tensor([5, 9, 1, 12], device="cuda")
    eager = HybridEngine(m, 4, 40, use_graph=False, fused_kv_append=fused, rollout_weights=mode)
    graph = HybridEngine(m, 4, 40, use_graph=True, fused_kv_append=fused, rollout_weights=mode)
    assert torch.equal(graph.generate(prompts, 10, temperature=0), eager.generate(prompts, 10, temperature=0))
    a = eager.generate_ragged(prompts, lens, 10, temperature=0)
    b = graph.generate_ragged(prompts, lens, 10, temperature=0)
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2])


@torch.no_grad()
@pytest.mark.parametrize("mode", FORMS)
def test_engine_owns_the_split_k_scratch(mode):
    """K = 1024 splits in two: the scratch is the engine's, sized by the eager
    step, and recording the graph on a fresh stream allocates none."""
    from dlrover_wuqiong_amd.ops import _hip

    torch.manual_seed(0)
    cfg = LlamaConfig(vocab_size=256, hidden_size=1024, intermediate_size=1024, num_hidden_layers=1,
                      num_attention_heads=8, num_key_value_heads=4, max_position_embeddings=128)
    with torch.device("cuda"):
        m = Llama(cfg)
    m = m.to(torch.bfloat16).eval()
    assert skinny_gemm.workspace_floats(4, 2048, 1024, mode == "fp8") > 0
    prompts = torch.randint(1, cfg.vocab_size, (4, 8), device="cuda")
    eager = HybridEngine(m, 4, 32, use_graph=False, rollout_weights=mode)
    graph = HybridEngine(m, 4, 32, use_graph=True, rollout_weights=mode)
    before = dict(_hip._SPLITK_WS)
    want = eager.generate(prompts, 8, temperature=0)
    got = graph.generate(prompts, 8, temperature=0)
    assert torch.equal(got, want)
    assert _hip._SPLITK_WS == before
    ws = graph._gemm_ws
    assert ws is not None and ws.numel() >= skinny_gemm.workspace_floats(4, 2048, 1024, mode == "fp8")
    graph.generate(prompts, 8, temperature=0)
    assert graph._gemm_ws is ws


@torch.no_grad()
def test_engine_fp8_copies_are_refreshed():
    m = _model()
    prompts = torch.randint(1, m.cfg.vocab_size, (4, 7), device="cuda")
    eng = HybridEngine(m, 4, 32, use_graph=False, rollout_weights="fp8")
    first = []
    forward = eng._forward

    def spy(ids, prefill, last=None):
        out = forward(ids, prefill=prefill, last=last)
        if not prefill:
            first.append(out.clone())
        return out

    eng._forward = spy
    eng.generate(prompts, 3, temperature=0)
    o_proj = m.layers[0].self_attn.o_proj
    codes, scale = eng._wq[o_proj]
    ptrs = (codes.data_ptr(), scale.data_ptr())
    before = (codes[3].float() * scale[3]).clone()
    n_steps = len(first)
    o_proj.weight[3] += 1.0
    eng.generate(prompts, 3, temperature=0)
    assert not torch.equal(first[n_steps], first[0])
    # the same buffers, refilled from the changed weight
    codes, scale = eng._wq[o_proj]
    assert (codes.data_ptr(), scale.data_ptr()) == ptrs
    after = codes[3].float() * scale[3]
    w = o_proj.weight[3].float()
    assert ((after - w).abs() <= 2.0 ** -4 * w.abs() + 2.0 ** -10 * scale[3]).all()
    assert float((after - before).mean()) > 0.9
