"""Weight-streaming decode GEMM, CPU side: the torch forms of
``ops.skinny_gemm`` (they define what the HIP kernels compute) and the hybrid
engine's ``rollout_weights`` option on CPU tensors."""

import copy

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from dlrover_wuqiong_amd.atorch.rl.config import PPOConfig
from dlrover_wuqiong_amd.atorch.rl.hybrid_engine import HybridEngine
from dlrover_wuqiong_amd.models.llama import Llama, LlamaConfig
from dlrover_wuqiong_amd.ops.skinny_gemm import quantize_rows_e4m3, skinny_linear


def test_quantize_rows_fallback():
    torch.manual_seed(0)
    w = (torch.randn(37, 96) * torch.logspace(-3, 2, 37)[:, None]).to(torch.bfloat16)
    w[5] = 0
    codes, scale = quantize_rows_e4m3(w)
    assert codes.dtype == torch.float8_e4m3fn and codes.shape == w.shape
    assert scale.dtype == torch.float32 and scale.shape == (37,)
    amax = w.float().abs().amax(1)
    want = amax / 448
    want[5] = 1.0
    assert torch.equal(scale, want)
    assert (codes[5].float() == 0).all()
    # half an e4m3 step (3 mantissa bits) + half the smallest subnormal (2^-9) of the scaled value
    err = (codes.float() * scale[:, None] - w.float()).abs()
    assert (err <= 2.0 ** -4 * w.float().abs() + 2.0 ** -10 * scale[:, None]).all()
    # caller-owned buffers are refilled in place
    out = (torch.empty_like(codes), torch.empty_like(scale))
    got = quantize_rows_e4m3(w, out=out)
    assert got[0] is out[0] and got[1] is out[1]
    assert torch.equal(out[0].view(torch.uint8), codes.view(torch.uint8)) and torch.equal(out[1], scale)
    with pytest.raises(ValueError):
        quantize_rows_e4m3(w, out=(torch.empty(3, 3, dtype=torch.float8_e4m3fn), out[1]))


def test_skinny_linear_fallback_is_the_defining_expression():
    torch.manual_seed(1)
    x = torch.randn(2, 3, 96).to(torch.bfloat16)
    w = torch.randn(40, 96).to(torch.bfloat16)
    codes, scale = quantize_rows_e4m3(w)
    y = skinny_linear(x, codes, scale)
    assert y.dtype == torch.bfloat16 and y.shape == (2, 3, 40)
    assert torch.equal(y, ((x.float() @ codes.float().T) * scale).to(torch.bfloat16))
    assert torch.equal(skinny_linear(x, codes, scale, splits=3), y)
    assert torch.equal(skinny_linear(x, w), F.linear(x, w))
    with pytest.raises(ValueError):
        skinny_linear(x[..., :64], w)


class _QuantDecodeLinear(nn.Module):
    """A layer linear whose one-token (decode) calls compute the defining
    expression on an e4m3 copy; longer inputs (prefill) keep ``F.linear``."""

    def __init__(self, lin):
        super().__init__()
        self.weight = lin.weight
        self.codes, self.scale = quantize_rows_e4m3(lin.weight.detach())

    def forward(self, x):
        if x.shape[-2] != 1:
            return F.linear(x, self.weight)
        return ((x.float() @ self.codes.float().T) * self.scale).to(x.dtype)


def _teacher_forced(eng, prompts, toks):
    eng._ensure_cache(prompts.shape[0], prompts.device, eng.llama.embed_tokens.weight.dtype)
    eng._refresh_rollout_weights()
    out = [eng._forward(prompts, prefill=True)]
    for t in range(toks.shape[1]):
        out.append(eng._forward(toks[:, t:t + 1], prefill=False).clone())
    return torch.stack(out)


@torch.no_grad()
def test_engine_rollout_weights_cpu():
    torch.manual_seed(0)
    m = Llama(LlamaConfig.named("llama-tiny")).eval()
    prompts = torch.randint(0, 1024, (3, 6))
    toks = torch.randint(0, 1024, (3, 4))
    base = _teacher_forced(HybridEngine(m, 4, 32), prompts, toks)
    assert torch.equal(_teacher_forced(HybridEngine(m, 4, 32, rollout_weights="bf16"), prompts, toks), base)

    got = _teacher_forced(HybridEngine(m, 4, 32, rollout_weights="fp8"), prompts, toks)
    mq = copy.deepcopy(m)
    for layer in mq.layers:
        layer.self_attn.qkv_proj = _QuantDecodeLinear(layer.self_attn.qkv_proj)
        layer.self_attn.o_proj = _QuantDecodeLinear(layer.self_attn.o_proj)
        layer.mlp.gate_up_proj = _QuantDecodeLinear(layer.mlp.gate_up_proj)
        layer.mlp.down_proj = _QuantDecodeLinear(layer.mlp.down_proj)
    want = _teacher_forced(HybridEngine(mq, 4, 32), prompts, toks)
    assert torch.equal(got, want)
    assert torch.equal(got[0], base[0])        # prefill keeps the bf16 / fp32 weights
    assert not torch.equal(got[1:], base[1:])  # the decode steps do run the e4m3 copies

    # generate() refreshes the copies itself and returns tokens of the usual shape
    eng = HybridEngine(m, 4, 32, rollout_weights="fp8")
    assert eng.generate(prompts, 4, temperature=0).shape == (3, 10)
    assert len(eng._wq) == 4 * m.cfg.num_hidden_layers


def test_engine_rollout_weights_rejects_tp_moe_and_unknown(monkeypatch):
    torch.manual_seed(0)
    moe = Llama(LlamaConfig.named("llama-moe-tiny"))
    with pytest.raises(ValueError, match="MoE"):
        HybridEngine(moe, 2, 16, rollout_weights="fp8")
    HybridEngine(moe, 2, 16)  # unset: MoE actors keep working
    m = Llama(LlamaConfig.named("llama-tiny"))
    with pytest.raises(ValueError, match="rollout_weights"):
        HybridEngine(m, 2, 16, rollout_weights="int4")
    # a tensor-parallel actor: its group spans two ranks
    import dlrover_wuqiong_amd.models.llama as llama_mod

    m.tp_group = object()
    monkeypatch.setattr(llama_mod, "_ws", lambda g: 2 if g is m.tp_group else 1)
    for mode in ("bf16", "fp8"):
        with pytest.raises(ValueError, match="tensor-parallel"):
            HybridEngine(m, 2, 16, rollout_weights=mode)


@torch.no_grad()
def test_engine_rollout_weights_needs_plain_linears():
    """An unmerged LoRA adapter (or a bias) is part of what the module
    computes: the streaming modes must not drop it from the decode steps."""
    from dlrover_wuqiong_amd.atorch.lora import apply_lora, merge_lora

    torch.manual_seed(0)
    m = Llama(LlamaConfig.named("llama-tiny")).eval()
    prompts = torch.randint(0, 1024, (2, 5))
    toks = torch.randint(0, 1024, (2, 3))
    late = HybridEngine(m, 2, 16, rollout_weights="bf16")   # built before the adapters exist
    plain = _teacher_forced(HybridEngine(m, 2, 16), prompts, toks)
    assert apply_lora(m, ["o_proj", "down_proj"], rank=4, freeze_others=False)
    for mod in m.modules():
        if hasattr(mod, "lora_B"):
            torch.nn.init.normal_(mod.lora_B, std=0.5)
    with_adapter = _teacher_forced(HybridEngine(m, 2, 16), prompts, toks)   # unset: adapters included
    assert not torch.allclose(with_adapter, plain)
    for mode in ("bf16", "fp8"):
        with pytest.raises(ValueError, match="LoraLinear"):
            HybridEngine(m, 2, 16, rollout_weights=mode)
    with pytest.raises(ValueError, match="LoraLinear"):
        _teacher_forced(late, prompts, toks)
    # merged adapters are plain linears again, and the streaming mode computes what the modules do
    merge_lora(m)
    for layer in m.layers:
        layer.self_attn.o_proj = layer.self_attn.o_proj.base
        layer.mlp.down_proj = layer.mlp.down_proj.base
    merged = _teacher_forced(HybridEngine(m, 2, 16), prompts, toks)
    assert torch.equal(_teacher_forced(HybridEngine(m, 2, 16, rollout_weights="bf16"), prompts, toks), merged)
    torch.testing.assert_close(merged, with_adapter, atol=1e-3, rtol=1e-3)
    # a bias is refused too
    m.layers[0].self_attn.o_proj = nn.Linear(256, 256, bias=True)
    with pytest.raises(ValueError, match="bias-free"):
        HybridEngine(m, 2, 16, rollout_weights="bf16")


@torch.no_grad()
def test_engine_fp8_decode_needs_its_copies():
    torch.manual_seed(0)
    m = Llama(LlamaConfig.named("llama-tiny")).eval()
    eng = HybridEngine(m, 2, 16, rollout_weights="fp8")
    prompts = torch.randint(0, 1024, (2, 5))
    eng.prefill(prompts)
    with pytest.raises(RuntimeError, match="e4m3 copy"):
        eng.decode(prompts[:, :1])   # no generate made the copies: never quietly the bf16 mode


def test_ppo_config_passes_rollout_weights():
    assert PPOConfig().rollout_weights is None
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
                              rollout_weights="fp8"))
    assert tr.train(1)
    assert tr._hy.rollout_weights == "fp8" and len(tr._hy._wq) == 4 * cfg.num_hidden_layers
