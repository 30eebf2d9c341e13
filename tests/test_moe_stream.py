"""``ops.moe_stream`` and the hybrid engine's ``moe_experts`` option on the
CPU: the torch expression against the MoE layer, validation, plumbing."""

import pytest
import torch

from dlrover_wuqiong_amd.atorch.rl.config import PPOConfig
from dlrover_wuqiong_amd.atorch.rl.hybrid_engine import HybridEngine
from dlrover_wuqiong_amd.models.llama import Llama, LlamaConfig
from dlrover_wuqiong_amd.ops.moe_stream import moe_stream_mlp


def _model(name="llama-moe-tiny"):
    torch.manual_seed(0)
    return Llama(LlamaConfig.named(name)).eval()


@torch.no_grad()
def test_matches_the_moe_layer():
    mlp = _model().layers[0].mlp
    x = torch.randn(11, mlp.experts.w1.shape[2])
    w, idx, _ = mlp.gate(x)
    got = moe_stream_mlp(x, w, idx, mlp.experts.w1, mlp.experts.w3, mlp.experts.w2)
    torch.testing.assert_close(got, mlp(x))


def test_option_validation():
    moe = _model()
    with pytest.raises(ValueError, match="moe_experts"):
        HybridEngine(moe, 2, 16, moe_experts="int8")
    with pytest.raises(ValueError, match="dense"):
        HybridEngine(_model("llama-tiny"), 2, 16, moe_experts="bf16")
    moe.layers[1].mlp.capacity_factor = 1.25
    with pytest.raises(ValueError, match="capacity_factor"):
        HybridEngine(moe, 2, 16, moe_experts="bf16")


def test_config_reaches_the_engine():
    from dlrover_wuqiong_amd.atorch.rl.trainer import PPOTrainer

    tr = PPOTrainer.__new__(PPOTrainer)
    tr.config = PPOConfig(rollout_moe_experts="fp8", max_new_tokens=4)
    tr.engine = type("E", (), {"actor": _model()})()
    hy = tr._hybrid(torch.zeros(2, 5, dtype=torch.long))
    assert hy.moe_experts == "fp8" and hy.use_graph


@torch.no_grad()
def test_cpu_generate_equals_the_module_path():
    m = _model()
    prompts = torch.randint(1, m.cfg.vocab_size, (3, 7))
    want = HybridEngine(m, 3, 24).generate(prompts, 8, temperature=0)
    assert torch.equal(HybridEngine(m, 3, 24, moe_experts="bf16").generate(prompts, 8, temperature=0), want)
    # the e4m3 copies are made and read (their tokens may differ: another policy)
    fp8 = HybridEngine(m, 3, 24, moe_experts="fp8")
    assert fp8.generate(prompts, 8, temperature=0).shape == want.shape and len(fp8._moe_q) == len(m.layers)
