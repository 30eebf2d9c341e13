"""PPO configuration.  Parity: ATorch ``atorch/rl/config.py`` (model
configs per role + PPO hyper-parameters: kl coefficient / adaptive target,
cliprange, cliprange_value, vf_coef, gamma, lam, ppo_epochs, whitening)."""

from dataclasses import dataclass
from typing import Optional


@dataclass
class PPOConfig:
    # generation
    max_new_tokens: int = 32
    temperature: float = 1.0
    top_k: int = 0
    top_p: float = 1.0
    # one fused, counter-based sampling launch per token (``ops.sampling``),
    # inside the captured decode graph on the GPU; seeded by ``seed``
    fused_sampling: bool = False
    # KV-cached generation from the training weights (Llama actors;
    # ``hybrid_engine.py``), HIP-graph decode on the GPU
    use_hybrid_engine: bool = True
    max_seq_len: Optional[int] = None   # cache length; default prompt + max_new_tokens
    # ragged rollouts: a response ends at ``eos_token_id`` (None: every row
    # generates max_new_tokens) and the rest of its row is ``pad_token_id``
    eos_token_id: Optional[int] = None
    pad_token_id: int = 0
    # QKV split + RoPE + K/V cache write of the decode step in one launch per
    # layer (``ops.rollout.kv_append_rope``; bf16 GPU Llama actors)
    fused_kv_append: bool = False
    # the decode step's GEMMs through the weight-streaming kernel
    # (``ops.skinny_gemm``): None (off) | "bf16" (the live weights) | "fp8"
    # (e4m3 copies of the layer weights, refilled at the start of every
    # rollout; the rollout policy then differs slightly from the bf16 one
    # that scores it: docs/rl_fp8_rollouts.md).  Dense single-rank actors.
    rollout_weights: Optional[str] = None
    # tokens between two host reads of the unfinished-row count (EOS stop)
    eos_check_interval: int = 8
    # rollout / optimisation
    rollout_batch_size: int = 16
    mini_batch_size: int = 8
    ppo_epochs: int = 4
    # objective
    init_kl_coef: float = 0.05
    target_kl: Optional[float] = None   # adaptive KL controller when set
    kl_horizon: int = 10000
    cliprange: float = 0.2
    cliprange_value: float = 0.2
    vf_coef: float = 0.5
    ent_coef: float = 0.0
    gamma: float = 1.0
    lam: float = 0.95
    whiten_advantages: bool = True
    scale_reward: Optional[str] = None   # None | "running" (divide by running std)
    max_grad_norm: float = 1.0
    actor_lr: float = 1e-5
    critic_lr: float = 1e-5
    seed: int = 0
    # Safe-RLHF style: reward - cost_coef * cost when the engine has a cost model
    cost_coef: float = 1.0
