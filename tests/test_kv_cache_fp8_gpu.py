"""GPU: the quantising K/V append (``dw_kv_append_rope_q8``) and the hybrid
engine's ``kv_cache="fp8"`` mode.  The cache's rule makes ``quantise(bf16
cache) == fp8 cache`` bit for bit, so both are checked with ``torch.equal``
against the bf16 path followed by the rule (quotients on the CPU: torch's GPU
division is one ulp low now and then)."""

import pytest
import torch

from dlrover_wuqiong_amd.atorch.rl.hybrid_engine import HybridEngine
from dlrover_wuqiong_amd.models.llama import Llama, LlamaConfig
from dlrover_wuqiong_amd.ops.rollout import kv_append_rope
from dlrover_wuqiong_amd.ops.rope import rope_table

pytestmark = pytest.mark.gpu
DEV = "cuda"
FP8 = torch.float8_e4m3fn


def _quant(x):
    """bf16 [..., D] -> (codes as uint8, scale fp32), on the CPU."""
    x = x.float().cpu()
    amax = x.abs().amax(-1)
    scale = torch.where(amax > 0, amax / 448.0, torch.ones_like(amax))
    return (x / scale[..., None]).clamp(-448, 448).to(FP8).view(torch.uint8), scale


@pytest.mark.parametrize("with_lens", [False, True])
@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("D", [64, 128])
def test_append_equals_quantised_bf16_append(D, S, with_lens):
    B, NH, NKV, Smax = 3, 4, 2, 11
    torch.manual_seed(D + S)
    qkv = torch.randn(B, S, NH + 2 * NKV, D, device=DEV).to(torch.bfloat16)
    qkv[1, 0, NH] = 0                                      # an all-zero K row: scale 1
    cos, sin = rope_table(32, D, 10000.0, DEV)
    lens = torch.tensor([0, 7, 10], device=DEV, dtype=torch.int32) if with_lens else None   # 10 + s >= 11: dropped
    kb, vb = torch.full((2, B, Smax + 2, 2 * NKV, D), float("nan"), device=DEV, dtype=torch.bfloat16)
    kb, vb = kb[:, :Smax, :NKV], vb[:, :Smax, :NKV]
    q_ref = kv_append_rope(qkv, NH, NKV, cos, sin, kb, vb, lens)
    kc, vc = torch.full((2, B, Smax + 2, 2 * NKV, D), 0x7F, device=DEV, dtype=torch.uint8).view(FP8)
    kc, vc = kc[:, :Smax, :NKV], vc[:, :Smax, :NKV]
    ks, vs = torch.full((2, B, 2 * NKV, Smax + 5), float("nan"), device=DEV)
    ks, vs = ks[:, :NKV, :Smax], vs[:, :NKV, :Smax]
    q = kv_append_rope(qkv, NH, NKV, cos, sin, kc, vc, lens, k_scale=ks, v_scale=vs)
    assert torch.equal(q, q_ref)
    for ref, codes, scale in ((kb, kc, ks), (vb, vc, vs)):
        written = ~ref.float().isnan().all(-1).cpu()       # [B, Smax, NKV]: what the bf16 kernel wrote
        assert int(written.sum()) == (B * S * NKV if not with_lens else (2 * S + 1) * NKV)
        want_c, want_s = _quant(torch.where(written[..., None].to(DEV), ref, torch.zeros_like(ref)))
        got_c, got_s = codes.view(torch.uint8).cpu(), scale.transpose(1, 2).cpu()
        assert torch.equal(got_c[written], want_c[written]) and torch.equal(got_s[written], want_s[written])
        assert bool((got_c[~written] == 0x7F).all()) and bool(got_s[~written].isnan().all())   # nothing else


def _model():
    torch.manual_seed(0)
    with torch.device(DEV):
        m = Llama(LlamaConfig.named("llama-tiny"))
    return m.to(torch.bfloat16).eval()


@torch.no_grad()
def test_engine_fp8_cache_graph_layout_and_size():
    m = _model()
    cfg = m.cfg
    Bq, P, T, Smax = 3, 5, 6, 15
    prompts = torch.randint(1, cfg.vocab_size, (Bq, P), device=DEV)
    toks = torch.randint(1, cfg.vocab_size, (Bq, T), device=DEV)

    def run(kv_cache, graph):
        eng = HybridEngine(m, Bq, Smax, use_graph=graph, fused_kv_append=True, kv_cache=kv_cache)
        out = [eng.prefill(prompts).clone(), eng._forward(toks[:, :1], prefill=False).clone()]   # eager: workspaces
        if graph:
            eng._capture(toks[:, 1:2])
        out += [eng.decode(toks[:, t:t + 1]).clone() for t in range(1, T)]
        return eng, torch.stack(out)

    eager, lg_eager = run("fp8", False)
    graphed, lg_graph = run("fp8", True)
    plain, lg_plain = run(None, False)
    assert torch.equal(lg_graph, lg_eager)                 # (a)
    c = eager.cache
    n = P + T                                              # (b) layer 0 does not depend on attention
    for ref, codes, scale in ((plain.cache.k, c.k, c.k_scale), (plain.cache.v, c.v, c.v_scale)):
        want_c, want_s = _quant(ref[0, :, :n])
        assert torch.equal(codes[0, :, :n].view(torch.uint8).cpu(), want_c)
        assert torch.equal(scale[0, :, :, :n].transpose(1, 2).cpu(), want_s)
    L, hkv, D = cfg.num_hidden_layers, cfg.num_key_value_heads, cfg.head_dim
    assert c.nbytes == 2 * L * Bq * Smax * hkv * D + 2 * L * Bq * hkv * 16 * 4   # (c) scales padded 15 -> 16
    print(f"[fp8 kv cache] max |logit diff| to the bf16-cache engine = "
          f"{float((lg_eager.float() - lg_plain.float()).abs().max()):.4f} "
          f"(max |logit| {float(lg_plain.float().abs().max()):.3f})")      # (d) recorded, not asserted
