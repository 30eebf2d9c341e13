"""CPU: ``Llama.forward(return_hidden=True)`` / ``head_weight()`` with
``linear_token_logprobs``, and ``PPOConfig.score_head`` through ``make_experience``."""

import pytest
import torch
import torch.nn.functional as F

from dlrover_wuqiong_amd.atorch.lora import apply_lora, merge_lora
from dlrover_wuqiong_amd.atorch.rl.config import PPOConfig
from dlrover_wuqiong_amd.atorch.rl.engine import ModelEngine, ValueModel
from dlrover_wuqiong_amd.atorch.rl.rl_config import AtorchRLConfig
from dlrover_wuqiong_amd.atorch.rl.trainer import PPOTrainer
from dlrover_wuqiong_amd.models.llama import Llama, LlamaConfig
from dlrover_wuqiong_amd.ops.token_stats import linear_token_logprobs, token_logprobs


def _cfg(tied=False):
    return LlamaConfig(vocab_size=61, hidden_size=32, intermediate_size=64, num_hidden_layers=2,
                       num_attention_heads=4, num_key_value_heads=2, max_position_embeddings=64,
                       tie_word_embeddings=tied)


@pytest.mark.parametrize("tied", [False, True])
def test_hidden_and_head_weight_give_the_models_statistics(tied):
    torch.manual_seed(0)
    model = Llama(_cfg(tied)).eval()
    ids = torch.randint(0, 61, (2, 9))
    labels = torch.randint(0, 61, (2, 9))
    labels[0, 3] = -100
    with torch.no_grad():
        h = model(ids, return_hidden=True)
        got = linear_token_logprobs(h, model.head_weight(), labels, True)
        want = token_logprobs(model(ids), labels, True)
    assert h.shape == (2, 9, 32) and got[0][0, 3] == 0
    assert (model.head_weight() is model.embed_tokens.weight) == tied
    for g, w in zip(got, want):
        torch.testing.assert_close(g, w, atol=1e-5, rtol=1e-5)


def test_gradient_route_matches_autograd_through_the_logits():
    torch.manual_seed(1)
    h0, w0 = torch.randn(3, 5, 16), torch.randn(23, 16) * 0.5
    labels = torch.randint(0, 23, (3, 5))
    grads = []
    for fn in (lambda h, w: linear_token_logprobs(h, w, labels, True),
               lambda h, w: token_logprobs(F.linear(h, w), labels, True)):
        h, w = h0.clone().requires_grad_(), w0.clone().requires_grad_()
        lp, ent = fn(h, w)
        (lp.sum() + 0.3 * ent.sum()).backward()
        grads.append((h.grad, w.grad))
    assert grads[0][0].abs().sum() > 0 and grads[0][1].abs().sum() > 0
    torch.testing.assert_close(grads[0], grads[1], atol=1e-6, rtol=1e-5)


@pytest.mark.parametrize("ragged,lora", [(False, None), (True, None), (False, "adapter"), (True, "merged")])
def test_make_experience_fused_scores_like_the_logits_path(ragged, lora):
    """``lora``: the actor's head carries an adapter with B != 0.  Unmerged,
    its weight alone is not the head, so the actor keeps the logits path."""
    stored = []
    for score_head in (None, "fused"):
        torch.manual_seed(0)
        cfg = _cfg()
        actor, ref, critic = Llama(cfg), Llama(cfg), ValueModel(Llama(cfg), cfg.vocab_size)
        if lora:
            assert apply_lora(actor, ["lm_head"], rank=2) == ["lm_head"]
            torch.nn.init.normal_(actor.lm_head.lora_B, std=0.5)
            if lora == "merged":
                merge_lora(actor)
        eng = ModelEngine(actor, critic, ref, lambda seq: seq.float().mean(1) / cfg.vocab_size, actor_lr=1e-4,
                          critic_lr=1e-4)
        tr = PPOTrainer(eng, torch.randint(0, cfg.vocab_size, (4, 5)),
                        PPOConfig(max_new_tokens=4, rollout_batch_size=4, mini_batch_size=2, ppo_epochs=1, seed=3,
                                  score_head=score_head))
        eng.eval()
        prompts = torch.randint(1, cfg.vocab_size, (4, 5))
        tr.make_experience(prompts, torch.tensor([5, 3, 4, 2]) if ragged else None)
        stored.append(tr.buffer.items[0])
        with torch.no_grad():   # which models took the fused route
            fused = [tr._fused_head(m) is not None for m in (actor, ref)]
            stats = tr._response_stats(ref, stored[-1].sequences, 5)
        assert fused == [score_head == "fused" and lora != "adapter", score_head == "fused"]
        assert (stats[0] is None) == (score_head == "fused")
    a, b = stored
    assert torch.equal(a.sequences, b.sequences)
    for k in ("logprobs", "advantages", "returns"):
        torch.testing.assert_close(getattr(b, k), getattr(a, k), atol=2e-5, rtol=1e-4)


def test_unknown_score_head_is_rejected():
    with pytest.raises(ValueError, match="score_head"):
        PPOConfig(score_head="fast")
    yaml = lambda v: AtorchRLConfig.from_dict({"model": {}, "method": {"PPOConfig": {"score_head": v}}})  # noqa: E731
    assert yaml("fused").to_ppo_config().score_head == "fused"
    assert AtorchRLConfig.from_dict({"model": {}}).to_ppo_config().score_head is None
    with pytest.raises(ValueError, match="score_head"):
        yaml("fast").to_ppo_config()
