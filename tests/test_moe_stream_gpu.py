"""Weight-streaming expert FFN on the GPU (``csrc/kernels/moe_stream.hip``):
a bound against fp64 over forms, routings and every tile / tail / split edge,
determinism and graph replay, and the hybrid engine's ``moe_experts`` modes."""

import functools

import pytest
import torch

from conftest import gpu_available
from dlrover_wuqiong_amd.atorch.rl.hybrid_engine import HybridEngine
from dlrover_wuqiong_amd.models.llama import Llama, LlamaConfig
from dlrover_wuqiong_amd.ops import moe_stream
from dlrover_wuqiong_amd.ops.moe_stream import moe_stream_mlp, moe_stream_mlp_ref, workspace_bytes

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a GPU")]

# (T, k, E, H, F): one tile; odd counts; a count across a 16-row group with an N tail in F and a K = 688 tile tail;
# 512 slots with 64 rows per expert; mostly empty experts with a K = 320 tail; a down K that splits
SHAPES = [(1, 1, 2, 32, 16), (5, 2, 4, 96, 48), (17, 2, 3, 256, 688), (64, 8, 8, 64, 64), (8, 2, 64, 320, 112),
          (4, 2, 4, 64, 2080)]
FORMS = ["bf16", "fp8"]
ROUTINGS = ["topk", "first_k", "dropped"]
U = 2.0 ** -24


@functools.lru_cache(maxsize=None)
def _case(shape, form, routing):
    """Inputs, the fp64 reference and the bound of
    ``test_bound_against_fp64`` (from the inputs and the reference only)."""
    T, k, E, H, F = shape
    g = torch.Generator(device="cuda").manual_seed(sum(shape))
    x = torch.randn(T, H, device="cuda", generator=g).to(torch.bfloat16)
    ws = [torch.randn(E, F, H, device="cuda", generator=g) / H ** 0.5 for _ in range(2)]
    ws.append(torch.randn(E, H, F, device="cuda", generator=g) / F ** 0.5)
    if routing == "first_k":
        idx = torch.arange(k, device="cuda").expand(T, k).contiguous()
        w = torch.rand(T, k, device="cuda", generator=g)
    else:
        w, idx = torch.randn(T, E, device="cuda", generator=g).softmax(-1).topk(k)
    w = w / w.sum(-1, keepdim=True)
    if routing == "dropped":
        drop = torch.rand(T, k, device="cuda", generator=g) < 0.3
        drop[0, 0] = True   # T = k = 1: every expert is empty and y is 0
        idx, w = idx.masked_fill(drop, E), w.masked_fill(drop, 0.0)
    if form == "fp8":
        # quantised with torch, so the reference sees the codes times the scales
        scales = tuple(t.abs().amax(2) / 448 for t in ws)
        ws = [(t / s[..., None]).clamp(-448, 448).to(torch.float8_e4m3fn) for t, s in zip(ws, scales)]
        d1, d3, d2 = (t.double() * s.double()[..., None] for t, s in zip(ws, scales))
    else:
        scales = None
        ws = [t.to(torch.bfloat16) for t in ws]
        d1, d3, d2 = (t.double() for t in ws)
    e = idx.clamp(max=E - 1)
    xd, wd = x.double(), (w.double() * (idx < E))

    def mm(a, m, eq):
        return torch.einsum(eq, a, m), torch.einsum(eq, a.abs(), m.abs())

    gt, a1 = mm(xd, d1[e], "th,tkfh->tkf")
    up, a3 = mm(xd, d3[e], "th,tkfh->tkf")
    eg, eu = (H + 1) * U * a1, (H + 1) * U * a3
    sg = torch.nn.functional.silu(gt)
    h = sg * up
    ds = 1.1 * eg + 2.0 ** -16 * (sg.abs() + 1.1 * eg)
    dpre = up.abs() * ds + sg.abs() * eu + ds * eu + U * h.abs()
    eh = dpre + 2.0 ** -8 * (h.abs() + dpre)
    z = torch.einsum("tkf,tknf->tkn", h, d2[e])
    ez = torch.einsum("tkf,tknf->tkn", eh, d2[e].abs()) \
        + (F + 17) * U * torch.einsum("tkf,tknf->tkn", h.abs() + eh, d2[e].abs())
    ref = (wd[..., None] * z).sum(1)
    bound = 2.0 ** -8 * ref.abs() + (1 + 2.0 ** -8) * (wd[..., None] * (ez + (k + 2) * U * (z.abs() + ez))).sum(1)
    return (x, w, idx, *ws, scales), ref, bound


@pytest.mark.parametrize("routing", ROUTINGS)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_bound_against_fp64(shape, form, routing):
    """With u = 2^-24, A = sum |x| |w| (scale included) and every quantity but
    y taken from the fp64 reference, stage by stage in the form of
    ``test_skinny_gemm_gpu.py``:

    * gate / up: ``eg = (H + 1) u A1``, ``eu = (H + 1) u A3`` (fp32
      accumulation over H and the scale's multiply);
    * silu: ``ds = 1.1 eg + 2^-16 (|silu g| + 1.1 eg)`` (|silu'| < 1.1; the
      hardware exp, the add and the divide stay within 2^-16 relative);
    * the product and h's one rounding: ``dpre = |up| ds + |silu g| eu + ds eu
      + u |h|``, ``eh = dpre + 2^-8 (|h| + dpre)``;
    * down: ``ez = |W2| eh + (F + 17) u |W2| (|h| + eh)`` (fp32 accumulation
      over F, at most 16 slices and the scale's multiply);
    * combine: ``|y - ref| <= 2^-8 |ref| + (1 + 2^-8) sum_j w_j (ez_j + (k + 2)
      u (|z_j| + ez_j))``.

    The workspace is the caller's, NaN-filled, with a guard behind it."""
    args, ref, bound = _case(shape, form, routing)
    need = workspace_bytes(*shape)
    ws = torch.full((need + 256,), 0xFF, device="cuda", dtype=torch.uint8)   # bf16 and fp32 NaNs
    y = moe_stream_mlp(*args[:6], scales=args[6], workspace=ws)
    assert y.dtype == torch.bfloat16 and y.shape == ref.shape
    assert (ws[need:] == 0xFF).all()
    ratio = float(((y.double() - ref).abs() / bound.clamp_min(1e-300)).max())
    print(f"{shape} {form} {routing}: max err / bound = {ratio:.3f}")
    assert ratio <= 1.0   # NaN fails too
    with pytest.raises(ValueError, match="workspace"):
        moe_stream_mlp(*args[:6], scales=args[6], workspace=ws[:need - 16])


@pytest.mark.parametrize("form", FORMS)
def test_deterministic_and_graph_replay(form):
    args = _case((17, 2, 3, 256, 688), form, "topk")[0]
    ws = torch.empty(workspace_bytes(17, 2, 3, 256, 688), device="cuda", dtype=torch.uint8)
    a = moe_stream_mlp(*args[:6], scales=args[6])
    assert torch.equal(a, moe_stream_mlp(*args[:6], scales=args[6], workspace=ws))
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            out = moe_stream_mlp(*args[:6], scales=args[6], workspace=ws)
    torch.cuda.current_stream().wait_stream(s)
    for _ in range(3):
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, a)


# ------------------------------------------------------------------ engine
def _model():
    torch.manual_seed(0)
    with torch.device("cuda"):
        m = Llama(LlamaConfig.named("llama-moe-tiny"))
    return m.to(torch.bfloat16).eval()


@torch.no_grad()
@pytest.mark.parametrize("mode", FORMS)
def test_engine_graph_decode_equals_eager(mode):
    m = _model()
    prompts = torch.randint(1, m.cfg.vocab_size, (4, 12), device="cuda")
    lens = torch.tensor([5, 9, 1, 12], device="cuda")
    eager = HybridEngine(m, 4, 40, use_graph=False, moe_experts=mode)
    graph = HybridEngine(m, 4, 40, use_graph=True, moe_experts=mode)
    assert graph.use_graph
    assert torch.equal(graph.generate(prompts, 10, temperature=0), eager.generate(prompts, 10, temperature=0))
    a = eager.generate_ragged(prompts, lens, 10, temperature=0)
    b = graph.generate_ragged(prompts, lens, 10, temperature=0)
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2])


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
    real = moe_stream.moe_stream_mlp
    monkeypatch.setattr(moe_stream, "moe_stream_mlp", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    got = _teacher_forced(HybridEngine(m, 4, 32, use_graph=False, moe_experts=mode), prompts, toks)
    assert len(calls) == 6 * m.cfg.num_hidden_layers   # decode steps only: prefill keeps the module
    monkeypatch.setattr(moe_stream, "moe_stream_mlp",
                        lambda x, w, idx, w1, w3, w2, scales=None, workspace=None: moe_stream_mlp_ref(
                            x, w, idx, w1, w3, w2, scales))
    want = _teacher_forced(HybridEngine(m, 4, 32, use_graph=False, moe_experts=mode), prompts, toks)
    torch.testing.assert_close(got.float(), want.float(), atol=5e-2, rtol=5e-2)


@torch.no_grad()
def test_engine_fp8_copies_are_refreshed():
    m = _model()
    prompts = torch.randint(1, m.cfg.vocab_size, (4, 7), device="cuda")
    eng = HybridEngine(m, 4, 32, use_graph=False, moe_experts="fp8")
    eng.generate(prompts, 3, temperature=0)
    mlp = m.layers[0].mlp
    codes, scale = eng._moe_q[mlp][2]
    ptrs = (codes.data_ptr(), scale.data_ptr())
    before = (codes[1, 3].float() * scale[1, 3]).clone()
    mlp.experts.w2[1, 3] += 1.0
    eng.generate(prompts, 3, temperature=0)
    codes, scale = eng._moe_q[mlp][2]
    assert (codes.data_ptr(), scale.data_ptr()) == ptrs
    after, wrow = codes[1, 3].float() * scale[1, 3], mlp.experts.w2[1, 3].float()
    assert ((after - wrow).abs() <= 2.0 ** -4 * wrow.abs() + 2.0 ** -10 * scale[1, 3]).all()
    assert float((after - before).mean()) > 0.9
