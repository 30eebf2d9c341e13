"""MXFP4 decode GEMM on the GPU: exact data for every chunk / tile / split seam, a float bound against fp64, the
block quantiser against its torch form, and the hybrid engine's ``rollout_weights="mxfp4"``."""

import functools

import pytest
import torch

from conftest import gpu_available
from dlrover_wuqiong_amd.atorch.rl.hybrid_engine import HybridEngine
from dlrover_wuqiong_amd.ops import skinny_gemm
from dlrover_wuqiong_amd.ops.skinny_gemm import (_quantize_mx_ref, dequantize_mxfp4, quantize_rows_mxfp4,
                                                  skinny_linear, skinny_linear_ref)
from test_skinny_gemm_mxfp4 import TIE_BLOCK, _model, _teacher_forced

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a GPU")]

# one block; less than one 128 chunk and N % 16 != 0; the 16-row boundary of M; 33 blocks (a chunk tail and a tile
# tail); 65 blocks (not divisible by the splits); M = 64 (the 256-deep tile, two of them); Llama-3's longest K
SHAPES = [(1, 16, 32), (5, 40, 96), (17, 48, 256), (16, 64, 1056), (33, 100, 2080), (64, 33, 512), (8, 272, 14336)]
SPLITS = [0, 1, 2, 3]
ids = {"ids": lambda s: "x".join(map(str, s))}


def _gen(shape):
    return torch.Generator(device="cuda").manual_seed(1000 * shape[0] + shape[1] + shape[2])


@functools.lru_cache(maxsize=None)
def _exact_case(shape):
    """Products are multiples of 2^-3, partial sums stay below 2^24 * 2^-3: fp32 is exact in any order."""
    M, N, K = shape
    g = _gen(shape)
    x = torch.randint(-2, 3, (M, K), device="cuda", generator=g).to(torch.bfloat16)
    codes = torch.randint(0, 256, (N, K // 2), device="cuda", generator=g).to(torch.uint8)
    scale = torch.randint(125, 129, (N, K // 32), device="cuda", generator=g).to(torch.uint8)
    w = dequantize_mxfp4(codes, scale).double()
    assert float((x.double().abs() @ w.abs().T).max()) < 2 ** 21
    return x, codes, scale, (x.double() @ w.T).to(torch.bfloat16)


@pytest.mark.parametrize("splits", SPLITS)
@pytest.mark.parametrize("shape", SHAPES, **ids)
def test_exact_data(shape, splits):
    x, codes, scale, want = _exact_case(shape)
    y = skinny_linear(x, codes, scale, splits=splits)
    assert y.dtype == torch.bfloat16 and y.shape == want.shape
    bad = (y != want).nonzero()
    assert bad.numel() == 0, (bad[:8].tolist(), y[tuple(bad[0])].item(), want[tuple(bad[0])].item())


@functools.lru_cache(maxsize=None)
def _float_case(shape):
    M, N, K = shape
    g = _gen(shape)
    x = torch.randn(M, K, device="cuda", generator=g).to(torch.bfloat16)
    # quantised with torch, so this test does not depend on the quantiser kernel
    codes, scale = _quantize_mx_ref(torch.randn(N, K, device="cuda", generator=g).to(torch.bfloat16))
    w = dequantize_mxfp4(codes, scale).double()
    return x, codes, scale, x.double() @ w.T, x.double().abs() @ w.abs().T


@pytest.mark.parametrize("splits", SPLITS)
@pytest.mark.parametrize("shape", SHAPES, **ids)
def test_float_bound_against_fp64(shape, splits):
    """|y - ref| <= 2^-8 |ref| (the bf16 rounding) + K 2^-24 A (1 + 2^-8) (worst-case fp32 accumulation),
    A = sum |x| |deq(w)|."""
    x, codes, scale, ref, A = _float_case(shape)
    y = skinny_linear(x, codes, scale, splits=splits)
    bound = 2.0 ** -8 * ref.abs() + shape[2] * 2.0 ** -24 * A * (1 + 2.0 ** -8)
    ratio = ((y.double() - ref).abs() / bound).max()
    print(f"{shape} splits={splits}: max err / bound = {float(ratio):.3f}")
    assert float(ratio) <= 1.0
    if shape == (17, 48, 256):
        assert torch.equal(skinny_linear(x, codes, scale, splits=splits), y)
        g, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            skinny_linear(x, codes, scale, splits=splits)   # the eager call that sizes the stream's workspace
            with torch.cuda.graph(g, stream=s):
                out = skinny_linear(x, codes, scale, splits=splits)
        torch.cuda.current_stream().wait_stream(s)
        for _ in range(3):
            out.zero_()
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, y)


@pytest.mark.parametrize("shape", [(33, 672), (272, 4096), (4100, 64), (19, 96)], **ids)
def test_quantiser_kernel(shape):
    N, K = shape
    g = torch.Generator(device="cuda").manual_seed(7)
    w = (torch.randn(N, K, device="cuda", generator=g)
         * torch.logspace(-3, 1, N, device="cuda")[:, None]).to(torch.bfloat16)
    if shape == (19, 96):
        w[7, 32:64] = 0
        w[8, 64:] = torch.tensor(TIE_BLOCK, device="cuda")
        w[9, :32] = torch.tensor(TIE_BLOCK, device="cuda") * 2.0 ** -9
    # outputs are views into larger buffers: what lies beyond them stays untouched
    cb = torch.full((N * K // 2 + 64,), 0x5A, device="cuda", dtype=torch.uint8)
    sb = torch.full((N * K // 32 + 64,), 0x5A, device="cuda", dtype=torch.uint8)
    codes, scale = cb[:N * K // 2].view(N, K // 2), sb[:N * K // 32].view(N, K // 32)
    got = quantize_rows_mxfp4(w, out=(codes, scale))
    assert got[0].data_ptr() == codes.data_ptr() and got[1].data_ptr() == scale.data_ptr()
    assert (cb[N * K // 2:] == 0x5A).all() and (sb[N * K // 32:] == 0x5A).all()
    want_codes, want_scale = _quantize_mx_ref(w)
    assert torch.equal(scale, want_scale)
    # values, not nibbles: the sign of a zero is free
    assert torch.equal(dequantize_mxfp4(codes, scale), dequantize_mxfp4(want_codes, want_scale))
    c2, s2 = quantize_rows_mxfp4(w)
    assert torch.equal(c2, codes) and torch.equal(s2, scale)


# ------------------------------------------------------------------ engine
@torch.no_grad()
def test_engine_decode_logits_match_torch_math(monkeypatch):
    m = _model("cuda", torch.bfloat16)
    prompts = torch.randint(1, m.cfg.vocab_size, (4, 9), device="cuda")
    toks = torch.randint(1, m.cfg.vocab_size, (4, 6), device="cuda")
    calls = []
    real = skinny_gemm.skinny_linear
    monkeypatch.setattr(skinny_gemm, "skinny_linear", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    got = _teacher_forced(HybridEngine(m, 4, 32, use_graph=False, rollout_weights="mxfp4"), prompts, toks)
    assert len(calls) == 6 * (4 * m.cfg.num_hidden_layers + 1)
    monkeypatch.setattr(skinny_gemm, "skinny_linear",
                        lambda x, w, scale=None, splits=0, workspace=None: skinny_linear_ref(x, w, scale))
    want = _teacher_forced(HybridEngine(m, 4, 32, use_graph=False, rollout_weights="mxfp4"), prompts, toks)
    torch.testing.assert_close(got.float(), want.float(), atol=5e-2, rtol=5e-2)


@torch.no_grad()
@pytest.mark.parametrize("fused", [False, True], ids=["unfused_kv", "fused_kv"])
def test_engine_graph_decode_equals_eager(fused):
    m = _model("cuda", torch.bfloat16)
    prompts = torch.randint(1, m.cfg.vocab_size, (4, 12), device="cuda")
    lens = torch.tensor([5, 9, 1, 12], device="cuda")
    eager = HybridEngine(m, 4, 40, use_graph=False, fused_kv_append=fused, rollout_weights="mxfp4")
    graph = HybridEngine(m, 4, 40, use_graph=True, fused_kv_append=fused, rollout_weights="mxfp4")
    assert torch.equal(graph.generate(prompts, 10, temperature=0), eager.generate(prompts, 10, temperature=0))
    a = eager.generate_ragged(prompts, lens, 10, temperature=0)
    b = graph.generate_ragged(prompts, lens, 10, temperature=0)
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2])
