"""CPU: the e4m3 KV cache's torch fallbacks (``decode_attention`` and
``kv_append_rope`` with scales) against the written-out fp64 expression, and
the engine / config option."""

import math

import pytest
import torch
import torch.nn as nn

from dlrover_wuqiong_amd.atorch.rl.config import PPOConfig
from dlrover_wuqiong_amd.atorch.rl.hybrid_engine import HybridEngine
from dlrover_wuqiong_amd.models.llama import Llama, LlamaConfig
from dlrover_wuqiong_amd.ops._hip import HipKernelError
from dlrover_wuqiong_amd.ops.attention import decode_attention
from dlrover_wuqiong_amd.ops.rollout import kv_append_rope
from dlrover_wuqiong_amd.ops.rope import apply_rope, rope_table

FP8 = torch.float8_e4m3fn


def _quant64(x):
    """The rule, every quotient in fp32 as the rule says: [..., D] -> codes, scale."""
    amax = x.float().abs().amax(-1)
    scale = torch.where(amax > 0, amax / 448.0, torch.ones_like(amax))
    return (x.float() / scale[..., None]).clamp(-448, 448).to(FP8), scale


def test_decode_attention_fallback_with_scales():
    torch.manual_seed(0)
    B, H, HKV, D, Smax, lens = 2, 4, 2, 16, 9, (9, 4)
    q = torch.randn(B, H, D).to(torch.bfloat16)
    kc, ks = _quant64(torch.randn(B, Smax, HKV, D))
    vc, vs = _quant64(torch.randn(B, Smax, HKV, D))
    ks, vs = ks.transpose(1, 2).contiguous(), vs.transpose(1, 2).contiguous()   # [B, HKV, Smax]
    out = decode_attention(q, kc, vc, torch.tensor(lens, dtype=torch.int32), k_scale=ks, v_scale=vs)
    for b, n in enumerate(lens):
        k = (kc[b, :n].double() * ks[b, :, :n].double().t()[..., None]).repeat_interleave(H // HKV, dim=1)
        v = (vc[b, :n].double() * vs[b, :, :n].double().t()[..., None]).repeat_interleave(H // HKV, dim=1)
        s = torch.einsum("hd,nhd->hn", q[b].double(), k) / math.sqrt(D)
        ref = torch.einsum("hn,nhd->hd", s.softmax(-1), v)
        torch.testing.assert_close(out[b].double(), ref, atol=2e-2, rtol=2e-2)
    for bad in (dict(k_scale=ks), dict(v_scale=vs), {}):   # fp8 caches without both scales
        with pytest.raises(HipKernelError):
            decode_attention(q, kc, vc, torch.tensor(lens, dtype=torch.int32), **bad)
    with pytest.raises(HipKernelError):                    # scales without fp8 caches
        decode_attention(q, kc.float(), vc.float(), torch.tensor(lens, dtype=torch.int32), k_scale=ks, v_scale=vs)


def test_kv_append_rope_fallback_with_scales():
    torch.manual_seed(1)
    B, S, NH, NKV, D, Smax = 3, 2, 4, 2, 16, 6
    qkv = torch.randn(B, S, NH + 2 * NKV, D)
    cos, sin = rope_table(16, D, 10000.0, "cpu")
    lens = torch.tensor([0, 3, 5], dtype=torch.int32)      # row 2's second token is past the cache
    kc, vc = torch.full((2, B, Smax, NKV, D), 0x7F, dtype=torch.uint8).view(FP8)
    ks, vs = torch.full((2, B, NKV, Smax), float("nan"))
    q = kv_append_rope(qkv, NH, NKV, cos, sin, kc, vc, lens, k_scale=ks, v_scale=vs)
    pos = lens.long().view(B, 1) + torch.arange(S)
    assert torch.equal(q, apply_rope(qkv[:, :, :NH].contiguous(), cos, sin, pos.clamp(max=15)))
    k = apply_rope(qkv[:, :, NH:NH + NKV].contiguous(), cos, sin, pos.clamp(max=15))
    written = torch.zeros(B, Smax, dtype=torch.bool)
    for b in range(B):
        for s in range(S):
            p = int(pos[b, s])
            if p >= Smax:
                continue
            written[b, p] = True
            for x, codes, scale in ((k, kc, ks), (qkv[:, :, NH + NKV:], vc, vs)):
                wc, wsc = _quant64(x[b, s])
                assert torch.equal(codes[b, p].view(torch.uint8), wc.view(torch.uint8))
                assert torch.equal(scale[b, :, p], wsc)
    assert int(written.sum()) == B * S - 1
    for codes, scale in ((kc, ks), (vc, vs)):              # nothing else was touched
        assert bool((codes.view(torch.uint8)[~written] == 0x7F).all())
        assert bool(scale.transpose(1, 2)[~written].isnan().all())


def test_engine_option():
    m = Llama(LlamaConfig.named("llama-tiny")).eval()
    with pytest.raises(ValueError, match="kv_cache"):
        HybridEngine(m, 2, 16, kv_cache="bogus")
    # a CPU engine runs both fallbacks and stays close to the plain cache
    prompts, toks = torch.randint(0, 1024, (2, 5)), torch.randint(0, 1024, (2, 3))
    outs = []
    for mode in (None, "fp8"):
        eng = HybridEngine(m, 2, 15, kv_cache=mode)
        with torch.no_grad():
            lg = [eng.prefill(prompts)] + [eng.decode(toks[:, t:t + 1]).clone() for t in range(3)]
        outs.append(torch.stack(lg))
    c = eng.cache
    assert c.k.dtype == FP8 and c.k_scale.shape == (m.cfg.num_hidden_layers, 2, c.k.shape[3], 15)
    assert c.k_scale.stride(2) == 16 and c.nbytes == 2 * c.k.numel() + 2 * 4 * c.k_scale.numel() // 15 * 16
    torch.testing.assert_close(outs[1], outs[0], atol=0.1, rtol=0.1)


def test_ppo_config_passes_rollout_kv_cache():
    assert PPOConfig().rollout_kv_cache is None
    from dlrover_wuqiong_amd.atorch.rl.engine import ModelEngine, ValueModel
    from dlrover_wuqiong_amd.atorch.rl.trainer import PPOTrainer

    torch.manual_seed(0)
    cfg = LlamaConfig.named("llama-tiny")
    actor, ref = Llama(cfg), Llama(cfg)

    class Reward(nn.Module):
        def forward(self, ids):
            return (ids[:, -2:] % 5 == 0).float().mean(-1)

    eng = ModelEngine(actor, ValueModel(Llama(cfg), cfg.vocab_size), ref, Reward(), actor_lr=1e-4, critic_lr=1e-4)
    tr = PPOTrainer(eng, torch.randint(0, cfg.vocab_size, (4, 5)),
                    PPOConfig(max_new_tokens=3, rollout_batch_size=2, mini_batch_size=2, ppo_epochs=1,
                              rollout_kv_cache="fp8"))
    assert tr.train(1)
    assert tr._hy.kv_cache == "fp8" and tr._hy.cache.k.dtype == FP8
