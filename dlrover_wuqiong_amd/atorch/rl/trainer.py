"""PPO trainer: rollout (sample responses with the actor), score them with
the reward model, KL-penalise against the reference model, GAE, then
``ppo_epochs`` of clipped-objective updates over shuffled mini-batches.

    engine = ModelEngine(actor, ValueModel(critic_trunk, V), ref, reward_fn)
    trainer = PPOTrainer(engine, prompt_dataset, PPOConfig(...))
    trainer.train(num_rollouts=100)

Parity: ATorch ``atorch/rl/trainer/{rl_trainer,ppo_trainer}.py``
(``RLTrainer`` hooks: pre_make_experience / post_experience_generation /
pre_rl_training / post_rl_training, ``make_experience``, ``rl_training``,
``evaluate``, ``train``) and the replay buffer of ``rl/replay_buffer``.
"""

import inspect
import os
from dataclasses import dataclass
from typing import Dict, List, Optional

import torch

from ...common.log import logger
from .config import PPOConfig
from ...ops.rollout import rollout_step
from ...ops.sampling import sample_tokens
from .engine import ModelEngine
from .ppo_utils import (AdaptiveKLController, FixedKLController, gae_advantages_and_returns, kl_penalised_rewards,
                        logprobs_and_entropy, logprobs_of_labels, ppo_loss)


@torch.no_grad()
def sample(actor, prompts: torch.Tensor, max_new_tokens: int, temperature: float = 1.0, top_k: int = 0,
           generator: Optional[torch.Generator] = None, top_p: float = 1.0) -> torch.Tensor:
    """Autoregressive sampling (full-sequence forward per token; use a
    KV-cached HF ``generate`` for long responses)."""
    ids = prompts
    for _ in range(max_new_tokens):
        logits = actor(ids)[:, -1, :].float()
        if temperature <= 0:
            nxt = logits.argmax(-1, keepdim=True)
        elif top_p < 1.0:
            nxt = sample_tokens(logits, temperature, top_k, top_p, generator=generator)
        else:
            logits = logits / temperature
            if top_k:
                kth = logits.topk(top_k, dim=-1).values[:, -1:]
                logits = logits.masked_fill(logits < kth, float("-inf"))
            nxt = torch.multinomial(logits.softmax(-1), 1, generator=generator)
        ids = torch.cat([ids, nxt], 1)
    return ids


@torch.no_grad()
def sample_ragged(actor, prompts: torch.Tensor, prompt_lens: torch.Tensor, max_new_tokens: int,
                  temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0,
                  generator: Optional[torch.Generator] = None, eos_token_id: Optional[int] = None,
                  pad_token_id: int = 0):
    """``sample`` for left-aligned prompts of different lengths with an
    optional EOS; the contract of ``HybridEngine.generate_ragged``: returns
    ``(seq [B, Pmax + max_new_tokens], prompt_lens, response_lens)`` with
    ``seq[b] = prompt_b | response_b | pad...``.  One full forward per token
    over the columns in use; row ``b``'s logits are read at its own last
    token, which under causal attention never saw the cells to its right."""
    B, Pmax = prompts.shape
    dev = prompts.device
    prompt_lens = torch.as_tensor(prompt_lens, device=dev).to(torch.int64).view(B)
    if int(prompt_lens.min()) < 1 or int(prompt_lens.max()) > Pmax:
        raise ValueError(f"prompt_lens must lie in [1, {Pmax}]")
    L = Pmax + max_new_tokens
    real = torch.arange(Pmax, device=dev).view(1, Pmax) < prompt_lens.view(B, 1)
    seq = torch.full((B, L), int(pad_token_id), device=dev, dtype=torch.int64)
    seq[:, :Pmax] = torch.where(real, prompts.to(torch.int64), seq[:, :Pmax])
    lens = prompt_lens.to(torch.int32)
    finished = torch.zeros(B, device=dev, dtype=torch.int32)
    resp_len = torch.zeros(B, device=dev, dtype=torch.int32)
    n_active = torch.full((1,), B, device=dev, dtype=torch.int32)
    tok = torch.zeros(B, 1, device=dev, dtype=torch.int64)
    rows = torch.arange(B, device=dev)
    for _ in range(max_new_tokens):
        logits = actor(seq[:, :int(lens.max())])[rows, lens.to(torch.int64) - 1].float()
        if temperature <= 0:
            nxt = logits.argmax(-1, keepdim=True)
        else:
            nxt = sample_tokens(logits, temperature, top_k, top_p, generator=generator)
        rollout_step(nxt, lens, finished, resp_len, seq, tok, n_active, eos_token_id, pad_token_id)
        lens += 1
        if eos_token_id is not None and int(n_active) == 0:
            break
    return seq, prompt_lens, resp_len.to(torch.int64)


@dataclass
class Experience:
    sequences: torch.Tensor      # [B, P + R]
    logprobs: torch.Tensor       # [B, R]
    values: torch.Tensor         # [B, R]
    advantages: torch.Tensor     # [B, R]
    returns: torch.Tensor        # [B, R]
    mask: torch.Tensor           # [B, R]
    scores: torch.Tensor         # [B]
    # ragged rollouts: row b is prompt_b | response_b | pad and its response
    # window starts at column prompt_lens[b]; None: every prompt has P columns
    prompt_lens: Optional[torch.Tensor] = None   # [B]


class ReplayBuffer:
    def __init__(self):
        self.items: List[Experience] = []

    def push(self, e: Experience):
        self.items.append(e)

    def clear(self):
        self.items = []

    def minibatches(self, size: int, generator: Optional[torch.Generator] = None):
        seqs = torch.cat([e.sequences for e in self.items])
        fields = {k: torch.cat([getattr(e, k) for e in self.items]) for k in
                  ("logprobs", "values", "advantages", "returns", "mask")}
        if all(e.prompt_lens is not None for e in self.items):
            fields["prompt_lens"] = torch.cat([e.prompt_lens for e in self.items])
        n = seqs.shape[0]
        perm = torch.randperm(n, generator=generator)
        for i in range(0, n, size):
            idx = perm[i:i + size]
            yield seqs[idx], {k: v[idx] for k, v in fields.items()}


class RLTrainer:
    def __init__(self, engine: ModelEngine, prompt_dataset, config: PPOConfig):
        self.engine, self.dataset, self.config = engine, prompt_dataset, config
        self.buffer = ReplayBuffer()
        self.stats_history: List[Dict[str, float]] = []
        self._batch_lens = None

    # hooks (reference names)
    def pre_make_experience_hook(self):
        self.engine.eval()

    def post_experience_generation_hook(self):
        pass

    def pre_rl_training_hook(self):
        self.engine.train()

    def post_rl_training_hook(self):
        self.buffer.clear()

    def make_experience(self, prompts):
        raise NotImplementedError

    def rl_training(self):
        raise NotImplementedError

    def evaluate(self, prompts) -> float:
        self.engine.eval()
        seq = sample(self.engine.actor, prompts, self.config.max_new_tokens, temperature=0.0)
        return float(self.engine.reward_model(seq).float().mean())

    def _prompt_batches(self):
        n = len(self.dataset)
        g = torch.Generator().manual_seed(self.config.seed)
        while True:
            idx = torch.randperm(n, generator=g)
            for i in range(0, n - self.config.rollout_batch_size + 1, self.config.rollout_batch_size):
                batch = idx[i:i + self.config.rollout_batch_size]
                self._batch_lens = None
                if self.config.eos_token_id is not None and hasattr(self.dataset, "lens_of"):
                    # ragged rollouts: the prompts' true lengths go with them
                    self._batch_lens = self.dataset.lens_of(batch)
                yield torch.stack([self.dataset[int(j)] for j in batch])

    def train(self, num_rollouts: int, checkpoint_interval: int = 0,
              checkpoint_dir: Optional[str] = None) -> List[Dict[str, float]]:
        """``checkpoint_interval`` > 0 saves actor + critic (and their
        optimizers) to ``checkpoint_dir/rollout_{it}`` every that many
        rollouts (reference ``TrainConfig.checkpoint_interval``)."""
        batches = self._prompt_batches()
        for it in range(num_rollouts):
            self.pre_make_experience_hook()
            prompts = next(batches)
            dev = next(self.engine.actor.parameters()).device
            if self._batch_lens is not None:
                self.make_experience(prompts.to(dev), self._batch_lens.to(dev))
            else:
                self.make_experience(prompts.to(dev))
            self.post_experience_generation_hook()
            self.pre_rl_training_hook()
            stats = self.rl_training()
            self.post_rl_training_hook()
            stats["rollout"] = it
            self.stats_history.append(stats)
            if checkpoint_interval and checkpoint_dir and (it + 1) % checkpoint_interval == 0:
                self.engine.save(os.path.join(checkpoint_dir, f"rollout_{it + 1}"))
            logger.info(f"rollout {it}: {stats}")
        return self.stats_history


class PPOTrainer(RLTrainer):
    def __init__(self, engine: ModelEngine, prompt_dataset, config: PPOConfig):
        super().__init__(engine, prompt_dataset, config)
        self.kl_ctl = (AdaptiveKLController(config.init_kl_coef, config.target_kl, config.kl_horizon)
                       if config.target_kl else FixedKLController(config.init_kl_coef))
        self.gen = torch.Generator(device="cpu").manual_seed(config.seed)
        self._last = {}
        self._rollouts = 0
        self._lengths_kw = {}   # id(reward / cost model) -> its forward takes ``lengths``

    def _hybrid(self, prompts):
        """The actor's hybrid (KV-cache) engine, or None to sample with full
        forwards (non-Llama or tensor/sequence-parallel actors)."""
        c = self.config
        if not c.use_hybrid_engine:
            return None
        need = (prompts.shape[0], c.max_seq_len or prompts.shape[1] + c.max_new_tokens)
        hy = getattr(self, "_hy", None)
        if hy is None or hy.max_batch < need[0] or hy.max_len < need[1]:
            from .hybrid_engine import HybridEngine, find_llama

            llama = find_llama(self.engine.actor)
            if llama is None:  # not a Llama-family actor: full-forward sampling
                self.config.use_hybrid_engine = False
                return None
            hy = self._hy = HybridEngine(self.engine.actor, need[0], need[1], fused_kv_append=c.fused_kv_append,
                                          rollout_weights=c.rollout_weights)
        return hy

    @staticmethod
    def _windows(x, prompt_lens, R):
        """x [B, L - 1, ...] indexed by predicting column -> the [B, R]
        response windows: row b, step t reads column ``p_b - 1 + t``."""
        idx = (prompt_lens.view(-1, 1) - 1) + torch.arange(R, device=x.device)
        return x.gather(1, idx)

    def _row_stats(self, model, seq, prompt_lens, R, with_entropy=False):
        """``_response_stats`` for ragged rows: the statistics of the whole
        row (one call of the token-stats op), then each row's window."""
        logits = model(seq)
        if with_entropy:
            lp, ent = logprobs_and_entropy(logits[:, :-1, :], seq[:, 1:])
            return logits, self._windows(lp, prompt_lens, R), self._windows(ent, prompt_lens, R)
        return logits, self._windows(logprobs_of_labels(logits[:, :-1, :], seq[:, 1:]), prompt_lens, R), None

    @staticmethod
    def _takes_lengths(model) -> bool:
        fn = model.forward if isinstance(model, torch.nn.Module) else model
        try:
            return "lengths" in inspect.signature(fn).parameters
        except (TypeError, ValueError):
            return False

    def _score(self, model, seq, lengths):
        """Sequence scores of a reward / cost model; ``lengths`` (the real
        tokens of each row) go to models whose forward takes them."""
        takes = self._lengths_kw.get(id(model))
        if takes is None:
            takes = self._lengths_kw[id(model)] = self._takes_lengths(model)
        return (model(seq, lengths=lengths) if takes else model(seq)).float()

    @torch.no_grad()
    def _make_experience_ragged(self, prompts: torch.Tensor, prompt_lens: Optional[torch.Tensor]):
        """Rollout of prompts of different lengths that may end at an EOS.
        ``prompts`` are left-padded (``PromptDataset``) with ``prompt_lens``
        real tokens each, or dense when ``prompt_lens`` is None.  Rows are
        stored ``prompt | response | pad``: every scoring pass is the plain
        causal forward and only the windows are per row."""
        from .rl_config import left_align

        c, e = self.config, self.engine
        B, Pmax = prompts.shape
        if prompt_lens is None:
            prompt_lens = torch.full((B,), Pmax, device=prompts.device, dtype=torch.int64)
        else:
            prompt_lens = prompt_lens.to(device=prompts.device, dtype=torch.int64)
            prompts = left_align(prompts, prompt_lens)
        g = self.gen if prompts.device.type == "cpu" else None
        hy = self._hybrid(prompts)
        if hy is not None:
            seed = c.seed + self._rollouts
            seq, _, resp_lens = hy.generate_ragged(
                prompts, prompt_lens, c.max_new_tokens, c.temperature, c.top_k, c.top_p, generator=g,
                fused_sampling=c.fused_sampling, seed=seed, eos_token_id=c.eos_token_id,
                pad_token_id=c.pad_token_id, eos_check_interval=c.eos_check_interval)
        else:
            seq, _, resp_lens = sample_ragged(e.actor, prompts, prompt_lens, c.max_new_tokens, c.temperature,
                                              c.top_k, c.top_p, generator=g, eos_token_id=c.eos_token_id,
                                              pad_token_id=c.pad_token_id)
        self._rollouts += 1
        R = seq.shape[1] - Pmax
        mask = (torch.arange(R, device=seq.device).view(1, R) < resp_lens.view(B, 1)).float()
        # what lies behind a row's response was computed from pad cells: zero it
        logprobs = self._row_stats(e.actor, seq, prompt_lens, R)[1] * mask
        ref_logprobs = self._row_stats(e.ref_model, seq, prompt_lens, R)[1] * mask
        values = self._windows(e.critic(seq)[:, :-1].float(), prompt_lens, R) * mask
        lengths = prompt_lens + resp_lens
        scores = self._score(e.reward_model, seq, lengths)
        if e.cost_model is not None:
            cost = self._score(e.cost_model, seq, lengths)
            self._cost = float(cost.mean())
            scores = scores - c.cost_coef * cost
        rewards, mean_kl = kl_penalised_rewards(logprobs, ref_logprobs, scores, mask, self.kl_ctl.value)
        adv, ret = gae_advantages_and_returns(values, rewards, mask, c.gamma, c.lam, c.whiten_advantages)
        self.buffer.push(Experience(seq, logprobs, values, adv, ret, mask, scores, prompt_lens))
        self.kl_ctl.update(float(mean_kl), seq.shape[0])
        self._last = {"reward/mean": float(scores.mean()), "policy/mean_kl": float(mean_kl),
                      "kl_coef": self.kl_ctl.value}

    def _response_stats(self, model, seq, P, with_entropy=False):
        """(logits, response log-probs, response entropy or None); the
        response logits are read in place, once for both statistics."""
        logits = model(seq)
        resp_logits = logits[:, P - 1:-1, :]
        if with_entropy:
            return (logits,) + logprobs_and_entropy(resp_logits, seq[:, P:])
        return logits, logprobs_of_labels(resp_logits, seq[:, P:]), None

    @torch.no_grad()
    def make_experience(self, prompts: torch.Tensor, prompt_lens: Optional[torch.Tensor] = None):
        """``prompt_lens`` [B] (the real tokens of each left-padded prompt) or
        a configured ``eos_token_id`` select the ragged rollout."""
        c, e = self.config, self.engine
        if prompt_lens is not None or c.eos_token_id is not None:
            return self._make_experience_ragged(prompts, prompt_lens)
        P = prompts.shape[1]
        g = self.gen if prompts.device.type == "cpu" else None
        hy = self._hybrid(prompts)
        if hy is not None:
            # a fresh random stream per rollout for the counter-based sampler
            seed = c.seed + self._rollouts
            seq = hy.generate(prompts, c.max_new_tokens, c.temperature, c.top_k, generator=g, top_p=c.top_p,
                              fused_sampling=c.fused_sampling, seed=seed)
        else:
            seq = sample(e.actor, prompts, c.max_new_tokens, c.temperature, c.top_k, generator=g, top_p=c.top_p)
        self._rollouts += 1
        R = seq.shape[1] - P
        mask = torch.ones(seq.shape[0], R, device=seq.device)
        _, logprobs, _ = self._response_stats(e.actor, seq, P)
        _, ref_logprobs, _ = self._response_stats(e.ref_model, seq, P)
        values = e.critic(seq)[:, P - 1:-1].float()
        scores = e.reward_model(seq).float()
        if e.cost_model is not None:
            cost = e.cost_model(seq).float()
            self._cost = float(cost.mean())
            scores = scores - c.cost_coef * cost
        rewards, mean_kl = kl_penalised_rewards(logprobs, ref_logprobs, scores, mask, self.kl_ctl.value)
        adv, ret = gae_advantages_and_returns(values, rewards, mask, c.gamma, c.lam, c.whiten_advantages)
        self.buffer.push(Experience(seq, logprobs, values, adv, ret, mask, scores))
        self.kl_ctl.update(float(mean_kl), seq.shape[0])
        self._last = {"reward/mean": float(scores.mean()), "policy/mean_kl": float(mean_kl),
                      "kl_coef": self.kl_ctl.value}

    def rl_training(self) -> Dict[str, float]:
        c, e = self.config, self.engine
        P = self.buffer.items[0].sequences.shape[1] - self.buffer.items[0].logprobs.shape[1]
        agg: Dict[str, float] = {}
        n = 0
        for _ in range(c.ppo_epochs):
            for seq, mb in self.buffer.minibatches(c.mini_batch_size, self.gen):
                pl = mb.get("prompt_lens")
                if pl is None:
                    _, logprobs, ent = self._response_stats(e.actor, seq, P, with_entropy=bool(c.ent_coef))
                    values = e.critic(seq)[:, P - 1:-1].float()
                else:
                    R = mb["mask"].shape[1]
                    _, logprobs, ent = self._row_stats(e.actor, seq, pl, R, with_entropy=bool(c.ent_coef))
                    values = self._windows(e.critic(seq)[:, :-1].float(), pl, R)
                loss, st = ppo_loss(logprobs, values, mb["logprobs"], mb["values"], mb["advantages"], mb["returns"],
                                    mb["mask"], c.cliprange, c.cliprange_value, c.vf_coef, ent, c.ent_coef)
                e.actor_optimizer.zero_grad(set_to_none=True)
                e.critic_optimizer.zero_grad(set_to_none=True)
                loss.backward()
                if c.max_grad_norm:
                    torch.nn.utils.clip_grad_norm_(e.trainable_parameters("actor"), c.max_grad_norm)
                    torch.nn.utils.clip_grad_norm_(e.trainable_parameters("critic"), c.max_grad_norm)
                e.actor_optimizer.step()
                e.critic_optimizer.step()
                for k, v in st.items():
                    agg[k] = agg.get(k, 0.0) + v
                n += 1
        out = {k: v / max(1, n) for k, v in agg.items()}
        out.update(self._last)
        return out
