"""Ragged RL rollouts against the dense rollout they generalise (1 GPU).

A/B/C, alternating in one process, host clock around ``generate`` (prefill and
graph capture included, as in ``scripts/bench_rl_token_ops.py``) divided by the
new tokens:

  (a) ``HybridEngine.generate``                                  (dense)
  (b) ``generate_ragged``, all lengths equal, no EOS, ``fused_kv_append`` off
  (c) the same with ``fused_kv_append`` on

all with graph decode, ``fused_sampling``, ``top_k = 50``, ``top_p = 0.95``.
(b) against (a) is the price of the ragged bookkeeping, (c) against (b) what
the fused K/V append kernel is worth.

Ragged row: prompt lengths uniform in [16, 128], an EOS token, and
``eos_check_interval`` in {1, 8, 32}: tokens generated against decode steps
run.  A random-weight model has no token it emits now and then, so the row
scales the LM-head row of the EOS token (``--eos-scale``) until it does; the
draws are seeded, so the three intervals see the same responses.

    python scripts/bench_rl_ragged_rollout.py [--out profiles/r7/rl_ragged_rollout_ab.jsonl]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from dlrover_wuqiong_amd.atorch.rl.hybrid_engine import HybridEngine  # noqa: E402
from dlrover_wuqiong_amd.models.llama import Llama, LlamaConfig  # noqa: E402


def _clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), out


def _summary(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3),
            "runs": [round(x, 3) for x in v]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/r7/rl_ragged_rollout_ab.jsonl")
    ap.add_argument("--model", default="llama3-8b")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--prompt", type=int, default=128)
    ap.add_argument("--new", type=int, default=128)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--eos-scale", type=float, default=3.0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_rl_ragged_rollout.py measures on a GPU; none found")
    rows = []

    def emit(r):
        rows.append(r)
        print(json.dumps(r), flush=True)

    torch.manual_seed(0)
    cfg = LlamaConfig.named(a.model)
    with torch.device("cuda"):
        m = Llama(cfg)
    m = m.to(torch.bfloat16).eval()
    B, P, T = a.batch, a.prompt, a.new
    p = torch.randint(0, cfg.vocab_size, (B, P), device="cuda")
    full = torch.full((B,), P, device="cuda")
    kw = dict(temperature=1.0, top_k=50, top_p=0.95, fused_sampling=True, seed=1)
    off = HybridEngine(m, B, P + T, use_graph=True)
    on = HybridEngine(m, B, P + T, use_graph=True, fused_kv_append=True)
    variants = {
        "a_generate": lambda n: off.generate(p, n, **kw),
        "b_ragged": lambda n: off.generate_ragged(p, full, n, **kw)[0],
        "c_ragged_fused_kv_append": lambda n: on.generate_ragged(p, full, n, **kw)[0],
    }
    for fn in variants.values():
        fn(8)  # warm-up
    ms = {k: [] for k in variants}
    seqs = {}
    for _ in range(a.runs):
        for k, fn in variants.items():
            t, seqs[k] = _clock(lambda: fn(T))
            ms[k].append(t / T)
    emit({"bench": "rollout_abc", "model": a.model, "batch": B, "prompt": P, "new": T, "top_k": 50, "top_p": 0.95,
          "graph": True, "fused_sampling": True, "ms_per_token": {k: _summary(v) for k, v in ms.items()},
          "same_tokens_a_b": bool(torch.equal(seqs["a_generate"], seqs["b_ragged"])),
          "same_tokens_b_c": bool(torch.equal(seqs["b_ragged"], seqs["c_ragged_fused_kv_append"])),
          "note": "host clock around the call (prefill + capture included) / new tokens; alternating runs"})

    # ragged prompts with an EOS the model emits now and then
    g = torch.Generator().manual_seed(2)
    lens = torch.randint(16, P + 1, (B,), generator=g).cuda()
    eos = 7
    head = m.embed_tokens.weight if m.lm_head is None else m.lm_head.weight
    with torch.no_grad():
        head[eos] *= a.eos_scale
    for interval in (1, 8, 32):
        t_ms, steps, toks = [], None, None
        for _ in range(a.runs):
            t, (seq, _, rl) = _clock(lambda: on.generate_ragged(p, lens, T, eos_token_id=eos, pad_token_id=0,
                                                                eos_check_interval=interval, **kw))
            t_ms.append(t)
            steps, toks = on.token_steps, rl.tolist()
        emit({"bench": "ragged_eos", "model": a.model, "batch": B, "prompt_lens": lens.tolist(), "max_new": T,
              "eos_check_interval": interval, "eos_scale": a.eos_scale, "response_lens": toks,
              "tokens_generated": sum(toks), "token_steps_run": steps,
              "rows_ended_before_max_new": sum(x < T for x in toks), "rollout_ms": _summary(t_ms),
              "fused_kv_append": True,
              "note": "token_steps_run counts sample + rollout_step steps, each but the last followed by a forward"})
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
