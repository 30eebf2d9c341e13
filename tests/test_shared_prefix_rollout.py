"""CPU: several samples per prompt over a shared-prefix KV cache
(docs/rl_shared_prefix.md): the reference op, the engine against repeated
prompts (fp32 llama-tiny, greedy, seed 0), the errors and the PPO switch."""

import pytest
import torch

from dlrover_wuqiong_amd.atorch.rl.config import PPOConfig
from dlrover_wuqiong_amd.atorch.rl.engine import ModelEngine, ValueModel
from dlrover_wuqiong_amd.atorch.rl.hybrid_engine import HybridEngine
from dlrover_wuqiong_amd.atorch.rl.rl_config import AtorchRLConfig
from dlrover_wuqiong_amd.atorch.rl.trainer import PPOTrainer
from dlrover_wuqiong_amd.models.llama import Llama, LlamaConfig
from dlrover_wuqiong_amd.ops.attention import decode_attention_reference, decode_attention_shared_reference

N, NEW = 3, 6


def test_reference_equals_plain_reference_on_the_repeated_concatenated_cache():
    g = torch.Generator().manual_seed(0)
    Bp, n, H, HKV, D, P, S = 2, 3, 4, 2, 16, 7, 5
    q = torch.randn(Bp * n, H, D, generator=g)
    kp, vp = torch.randn(Bp, P, HKV, D, generator=g), torch.randn(Bp, P, HKV, D, generator=g)
    ks, vs = torch.randn(Bp * n, S, HKV, D, generator=g), torch.randn(Bp * n, S, HKV, D, generator=g)
    pl, sl = torch.tensor([7, 2], dtype=torch.int32), torch.tensor([0, 1, 5, 3, 0, 2], dtype=torch.int32)
    kc, vc = torch.zeros(Bp * n, P + S, HKV, D), torch.zeros(Bp * n, P + S, HKV, D)
    for b in range(Bp * n):
        a, s = int(pl[b // n]), int(sl[b])
        kc[b, :a + s] = torch.cat([kp[b // n, :a], ks[b, :s]])
        vc[b, :a + s] = torch.cat([vp[b // n, :a], vs[b, :s]])
    out = decode_attention_shared_reference(q, kp, vp, pl, ks, vs, sl, n)
    assert torch.equal(out, decode_attention_reference(q, kc, vc, pl.repeat_interleave(n) + sl))


@pytest.fixture(scope="module")
def model():
    torch.manual_seed(0)
    return Llama(LlamaConfig.named("llama-tiny")).eval()


def _prompts():
    return torch.randint(1, 1024, (2, 5), generator=torch.Generator().manual_seed(3))


def test_generate_equals_repeated_prompts(model):
    p = _prompts()
    ref = HybridEngine(model, 2 * N, 16).generate(p.repeat_interleave(N, 0), NEW, temperature=0.0)
    eng = HybridEngine(model, 2 * N, 16)
    out = eng.generate(p, NEW, temperature=0.0, samples_per_prompt=N)
    assert out.shape == (2 * N, 5 + NEW) and torch.equal(out, ref)
    assert eng.prefix.k.shape[1:3] == (2, 5) and eng.cache.k.shape[1:3] == (2 * N, NEW)
    # the engine goes back to one cache per row
    assert torch.equal(eng.generate(p, NEW, temperature=0.0), ref[::N])


def test_generate_ragged_equals_repeated_prompts(model):
    p, lens = _prompts(), torch.tensor([5, 3])
    kw = dict(temperature=0.0, pad_token_id=0, eos_check_interval=1)
    free = HybridEngine(model, 2 * N, 16).generate_ragged(p, lens, NEW, **kw)[0]
    eos = int(free[1, 3 + 2])   # row 1 stops after three tokens
    ref = HybridEngine(model, 2 * N, 16).generate_ragged(p.repeat_interleave(N, 0), lens.repeat_interleave(N), NEW,
                                                         eos_token_id=eos, **kw)
    out = HybridEngine(model, 2 * N, 16).generate_ragged(p, lens, NEW, eos_token_id=eos, samples_per_prompt=N, **kw)
    assert out[2][N:].tolist() == [3] * N
    for a, b in zip(out, ref):
        assert torch.equal(a, b)


@torch.no_grad()
def test_the_seed_has_no_argmax_near_tie(model):
    """The equalities above compare argmaxes of two fp32 evaluation orders."""
    seq = HybridEngine(model, 2, 16).generate(_prompts(), NEW, temperature=0.0)
    top = model(seq[:, :-1])[:, 4:].float().topk(2, -1).values
    assert float((top[..., 0] - top[..., 1]).min()) > 1e-3


@pytest.mark.parametrize("kw,word", [(dict(kv_cache="fp8"), "fp8"), (dict(fused_kv_append=True), "fused_kv_append"),
                                     (dict(), "tensor-parallel")])
def test_unsupported_combinations_raise_in_the_call(model, kw, word):
    eng = HybridEngine(model, 8, 16, **kw)
    if not kw:
        eng.tp = 2   # what a tensor-parallel actor sets
    p = _prompts()
    with pytest.raises(ValueError, match=word):
        eng.generate(p, NEW, temperature=0.0, samples_per_prompt=2)
    with pytest.raises(ValueError, match=word):
        eng.generate_ragged(p, torch.tensor([5, 3]), NEW, temperature=0.0, samples_per_prompt=2)


@pytest.mark.parametrize("hybrid", [True, False])
@pytest.mark.parametrize("eos", [None, 5])
def test_ppo_experience_has_n_rows_per_prompt(hybrid, eos):
    torch.manual_seed(0)
    cfg = LlamaConfig.named("llama-tiny")
    eng = ModelEngine(Llama(cfg), ValueModel(Llama(cfg), cfg.vocab_size), Llama(cfg),
                      lambda ids, lengths=None: ids.float().mean(1), actor_lr=1e-4, critic_lr=1e-4)
    eng.eval()
    pc = PPOConfig(max_new_tokens=4, rollout_batch_size=2, mini_batch_size=2, temperature=0.0, eos_token_id=eos,
                   samples_per_prompt=2, use_hybrid_engine=hybrid)
    tr = PPOTrainer(eng, None, pc)
    p = _prompts()
    tr.make_experience(p)
    e = tr.buffer.items[0]
    assert e.sequences.shape == (4, 9) and e.logprobs.shape == (4, 4) and e.scores.shape == (4,)
    assert torch.equal(e.sequences[:, :5], p.repeat_interleave(2, 0))
    assert torch.equal(e.sequences[0], e.sequences[1])   # greedy samples of one prompt


def test_yaml_generation_section_carries_samples_per_prompt():
    rc = AtorchRLConfig.from_dict({"model": {}, "generation": {"batch_size": 4, "samples_per_prompt": 4}})
    assert rc.to_ppo_config().samples_per_prompt == 4
    assert AtorchRLConfig.from_dict({"model": {}}).to_ppo_config().samples_per_prompt == 1
