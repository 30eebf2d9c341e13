"""CPU: the ``kernel`` option of ``decode_attention`` and its way through
``HybridEngine(decode_kernel=...)`` and ``PPOConfig.rollout_decode_kernel``."""

import pytest
import torch
import torch.nn as nn

from dlrover_wuqiong_amd.atorch.rl.config import PPOConfig
from dlrover_wuqiong_amd.atorch.rl.hybrid_engine import HybridEngine
from dlrover_wuqiong_amd.models.llama import Llama, LlamaConfig
from dlrover_wuqiong_amd.ops._hip import HipKernelError
from dlrover_wuqiong_amd.ops.attention import decode_attention, decode_attention_reference


def test_decode_attention_kernel_option_on_cpu():
    torch.manual_seed(0)
    B, H, HKV, D, Smax = 2, 4, 2, 16, 9
    q, k, v = torch.randn(B, H, D), torch.randn(B, Smax, HKV, D), torch.randn(B, Smax, HKV, D)
    lens = torch.tensor([9, 4], dtype=torch.int32)
    ref = decode_attention_reference(q, k, v, lens)
    for kernel in ("mfma", "valu"):
        assert torch.equal(decode_attention(q, k, v, lens, kernel=kernel), ref)
    with pytest.raises(ValueError, match="kernel"):
        decode_attention(q, k, v, lens, kernel="wmma")
    codes, scale = k.to(torch.float8_e4m3fn), torch.ones(B, HKV, Smax)
    fp8 = dict(k_scale=scale, v_scale=scale)
    assert torch.equal(decode_attention(q, codes, codes, lens, kernel="mfma", **fp8),
                       decode_attention_reference(q, codes, codes, lens, **fp8))
    with pytest.raises(HipKernelError, match="valu"):
        decode_attention(q, codes, codes, lens, kernel="valu", **fp8)


def test_engine_decode_kernel_option():
    torch.manual_seed(0)
    m = Llama(LlamaConfig.named("llama-tiny")).eval()
    with pytest.raises(ValueError, match="decode_kernel"):
        HybridEngine(m, 2, 16, decode_kernel="valu")
    prompts = torch.randint(0, 1024, (2, 5))
    seqs = [HybridEngine(m, 2, 16, decode_kernel=dk).generate(prompts, 6, temperature=0.0) for dk in (None, "mfma")]
    assert seqs[0].shape == (2, 11) and torch.equal(seqs[0], seqs[1])


def test_ppo_config_passes_rollout_decode_kernel():
    assert PPOConfig().rollout_decode_kernel is None
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
                              rollout_decode_kernel="mfma"))
    assert tr.train(1)
    assert tr._hy.decode_kernel == "mfma"
