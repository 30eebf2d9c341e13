"""RL rollout token ops on the CPU: the kept set of temperature / top-k /
top-p sampling against a brute-force fp64 computation, the torch math of
``ops.token_stats`` (bitwise the old ``ppo_utils`` expressions, hand-written
backward vs fp64 autograd), and the ``top_p`` plumbing from the YAML down to
the samplers."""

import math

import pytest
import torch
import torch.nn.functional as F

from dlrover_wuqiong_amd.ops.sampling import keep_mask, sample_tokens
from dlrover_wuqiong_amd.ops.token_stats import backward_math, token_entropy, token_logprobs

V = 4099
HEAD_P = (0.30, 0.20, 0.14, 0.09, 0.06, 0.04, 0.03, 0.02)
HEAD_IDX = (0, 7, 8, 255, 256, 2049, 4096, 4098)
# (temperature, top_k, top_p, kept): number of head tokens kept, None = every token
CASES = ((1.0, 0, 0.76, 5), (0.7, 0, 0.87, 4), (1.0, 5, 0.90, 4), (1.0, 5, 1.0, 5), (1.0, 20, 1.0, None))
MARGIN = 0.02


def fixture_logits(v=V):
    """One row: eight head tokens with the probabilities above, a uniform
    tail, logits = log-probabilities rounded to bf16.  ``v`` < 4099 keeps the
    head tokens that fit (indices below ``v``) and renormalises nothing: only
    the order and the gaps matter."""
    idx = [i for i in HEAD_IDX if i < v]
    p = torch.full((v,), (1.0 - sum(HEAD_P)) / (V - len(HEAD_IDX)), dtype=torch.float64)
    p[idx] = torch.tensor(HEAD_P[:len(idx)], dtype=torch.float64)
    return p.log().to(torch.bfloat16)


def brute_force(logits, temperature, top_k, top_p):
    """(kept mask, strictly-above mass per token) of one row, by an fp64 sort
    and an O(V^2) comparison."""
    z = (logits.float() / temperature).double()
    kept = torch.ones_like(z, dtype=torch.bool)
    if top_k:
        kth = z.sort(descending=True).values[top_k - 1]
        kept = z >= kth
    w = torch.where(kept, (z - z.max()).exp(), torch.zeros_like(z))
    w = w / w.sum()
    above = ((z.unsqueeze(0) > z.unsqueeze(1)) * w.unsqueeze(0)).sum(1)  # above[j] = sum_{z_i > z_j} w_i
    if top_p < 1.0:
        kept = kept & (above < top_p)
    return kept, above


def expected_kept(n_head):
    m = torch.zeros(V, dtype=torch.bool)
    if n_head is None:
        return ~m
    m[list(HEAD_IDX[:n_head])] = True
    return m


def test_fixture_masses():
    x = fixture_logits()
    for T, k, head in ((1.0, 0, (0, .300, .500, .640, .730, .790, .830, .860)),
                       (0.7, 0, (0, .435, .679, .825, .903)), (1.0, 5, (0, .380, .633, .810, .924))):
        _, above = brute_force(x, T, k, 1.0)
        for i, a in zip(HEAD_IDX, head):
            assert abs(float(above[i]) - a) < 5e-3, (T, k, i, float(above[i]), a)
    _, above = brute_force(x, 1.0, 0, 1.0)
    assert abs(float(above[1]) - 0.880) < 5e-3  # a tail token


@pytest.mark.parametrize("T,top_k,top_p,n_head", CASES)
def test_keep_mask_matches_brute_force(T, top_k, top_p, n_head):
    x = fixture_logits()
    kept, above = brute_force(x, T, top_k, top_p)
    if top_p < 1.0:
        # no mass within MARGIN of the cut: a reordered sum cannot move a token across it
        assert float((above - top_p).abs().min()) >= MARGIN
    assert torch.equal(kept, expected_kept(n_head))
    got = keep_mask(x.unsqueeze(0).repeat(3, 1), T, top_k, top_p)
    assert got.dtype == torch.bool and got.shape == (3, V)
    for r in range(3):
        assert torch.equal(got[r], kept)
    # fp32 logits of the same values define the same set
    assert torch.equal(keep_mask(x.float().unsqueeze(0), T, top_k, top_p)[0], kept)


def test_keep_mask_always_keeps_the_top_token():
    x = fixture_logits().unsqueeze(0)
    m = keep_mask(x, 1.0, 0, 1e-9)
    assert m.sum() == 1 and bool(m[0, 0])
    assert keep_mask(x, 1.0, 0, 1.0).all() and keep_mask(x, 1.0, V + 5, 1.0).all()


def test_sample_tokens_torch_path_only_emits_kept_tokens():
    x = fixture_logits().unsqueeze(0).repeat(512, 1)
    g = torch.Generator().manual_seed(0)
    for T, top_k, top_p, n_head in CASES[:3]:
        tok = sample_tokens(x, T, top_k, top_p, generator=g)
        assert tok.shape == (512, 1) and tok.dtype == torch.int64
        assert set(tok.view(-1).tolist()) <= set(HEAD_IDX[:n_head])
    assert sample_tokens(x, 0.0).view(-1).tolist() == [0] * 512


# ------------------------------------------------------------------ op math
def test_token_logprobs_cpu_is_bitwise_the_old_expressions():
    torch.manual_seed(0)
    full = (3 * torch.randn(2, 7, 131)).to(torch.bfloat16)
    for logits in (full[:, 1:-1], full.float()[:, 1:-1], full[0]):
        labels = torch.randint(0, 131, logits.shape[:-1])
        lp = F.log_softmax(logits.float(), dim=-1)
        old_logp = lp.gather(-1, labels.unsqueeze(-1)).squeeze(-1)
        old_ent = -(lp.exp() * lp).sum(-1)
        logp, ent = token_logprobs(logits, labels, with_entropy=True)
        assert logp.dtype == torch.float32 and logp.shape == labels.shape
        assert torch.equal(logp, old_logp) and torch.equal(ent, old_ent)
        assert torch.equal(token_logprobs(logits, labels), old_logp)
        assert torch.equal(token_entropy(logits), old_ent)


def test_token_logprobs_cpu_masked_vocabulary_and_ignored_label():
    torch.manual_seed(1)
    x = torch.randn(4, 33)
    x[:, ::3] = float("-inf")
    labels = torch.tensor([1, 2, -100, 40])
    logp, ent = token_logprobs(x, labels, with_entropy=True)
    assert torch.isfinite(ent).all() and torch.isfinite(logp).all()
    assert logp[2] == 0 and logp[3] == 0
    p = x.double().softmax(-1)
    ref = -(torch.where(p > 0, p * p.clamp_min(1e-300).log(), torch.zeros_like(p))).sum(-1)
    torch.testing.assert_close(ent.double(), ref, atol=1e-5, rtol=1e-5)


def test_backward_math_matches_fp64_autograd():
    torch.manual_seed(2)
    x = (2 * torch.randn(3, 5, 37, dtype=torch.float64)).requires_grad_()
    labels = torch.randint(0, 37, (3, 5))
    labels[1, 2] = -100
    g1 = torch.randn(3, 5, dtype=torch.float64)
    g2 = torch.randn(3, 5, dtype=torch.float64)
    lp = F.log_softmax(x, dim=-1)
    valid = labels >= 0
    logp = torch.where(valid, lp.gather(-1, labels.clamp_min(0).unsqueeze(-1)).squeeze(-1), torch.zeros_like(g1))
    ent = -(lp.exp() * lp).sum(-1)
    lse = torch.logsumexp(x, -1).detach()
    for a, b in ((g1, g2), (g1, None), (None, g2)):
        obj = (0 if a is None else (a * logp).sum()) + (0 if b is None else (b * ent).sum())
        ref, = torch.autograd.grad(obj, x, retain_graph=True)
        got = backward_math(x.detach(), labels, lse, ent.detach(), a, b)
        assert float((got - ref).abs().max()) < 1e-13
    # p = 0 (a -inf logit) gives 0, not NaN
    xm = x.detach().clone()
    xm[..., ::4] = float("-inf")
    lse = torch.logsumexp(xm, -1)
    p = xm.softmax(-1)
    ent = -(torch.where(p > 0, p * (xm - lse.unsqueeze(-1)), torch.zeros_like(p))).sum(-1)
    got = backward_math(xm, (labels.clamp_min(0) % 9) * 4 + 1, lse, ent, g1, g2)  # labels off the masked columns
    assert torch.isfinite(got).all() and (got[..., ::4] == 0).all()


# ------------------------------------------------------------------- config
def test_rl_config_passes_top_p():
    from dlrover_wuqiong_amd.atorch.rl.config import PPOConfig
    from dlrover_wuqiong_amd.atorch.rl.rl_config import AtorchRLConfig

    assert PPOConfig().top_p == 1.0 and PPOConfig().fused_sampling is False
    cfg = {"model": {"actor": {"model_cls": "x.Y"}, "critic": {"model_cls": "x.Y"}},
           "generation": {"batch_size": 4, "gen_experience_kwargs": {"max_new_tokens": 8, "do_sample": True,
                                                                      "temperature": 1.0, "top_k": 50, "top_p": 0.95}}}
    ppo = AtorchRLConfig.from_dict(cfg).to_ppo_config()
    assert ppo.top_p == 0.95 and ppo.top_k == 50 and ppo.temperature == 1.0
    del cfg["generation"]["gen_experience_kwargs"]["top_p"]
    assert AtorchRLConfig.from_dict(cfg).to_ppo_config().top_p == 1.0


class _Stub(torch.nn.Module):
    """Returns the fixture logits at every position."""

    def __init__(self):
        super().__init__()
        self.row = fixture_logits()

    def forward(self, ids):
        return self.row.expand(ids.shape[0], ids.shape[1], V)


def test_trainer_sample_with_top_p_only_emits_kept_tokens():
    from dlrover_wuqiong_amd.atorch.rl.trainer import sample

    prompts = torch.zeros(64, 2, dtype=torch.long)
    g = torch.Generator().manual_seed(3)
    seq = sample(_Stub(), prompts, 6, temperature=1.0, top_k=0, generator=g, top_p=0.76)
    assert seq.shape == (64, 8)
    drawn = set(seq[:, 2:].reshape(-1).tolist())
    assert drawn <= set(HEAD_IDX[:5]) and len(drawn) > 1
    # the default is today's path: same generator state, same tokens as top_p = 1 spelled out
    a = sample(_Stub(), prompts, 3, generator=torch.Generator().manual_seed(4))
    b = sample(_Stub(), prompts, 3, generator=torch.Generator().manual_seed(4), top_p=1.0)
    assert torch.equal(a, b)


def test_ppo_trainer_samples_with_config_top_p():
    """make_experience forwards top_p: with the stub actor every response
    token lies in the top_p = 0.76 kept set."""
    from dlrover_wuqiong_amd.atorch.rl.config import PPOConfig
    from dlrover_wuqiong_amd.atorch.rl.trainer import PPOTrainer

    class Engine:
        actor = ref_model = _Stub()
        cost_model = None

        @staticmethod
        def critic(seq):
            return torch.zeros(seq.shape, dtype=torch.float32)

        @staticmethod
        def reward_model(seq):
            return torch.zeros(seq.shape[0])

    cfg = PPOConfig(max_new_tokens=5, top_p=0.76, use_hybrid_engine=False, rollout_batch_size=16)
    tr = PPOTrainer(Engine(), [torch.zeros(2, dtype=torch.long)] * 16, cfg)
    tr.make_experience(torch.zeros(16, 2, dtype=torch.long))
    seq = tr.buffer.items[0].sequences
    assert set(seq[:, 2:].reshape(-1).tolist()) <= set(HEAD_IDX[:5])
    lp = tr.buffer.items[0].logprobs
    assert lp.shape == (16, 5) and float(lp.max()) <= math.log(0.31)
