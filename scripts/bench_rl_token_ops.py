"""RL rollout token ops against the torch chains they replace (1 GPU).

Sampler: ``ops.sampling.sample_tokens`` (one fused launch) against today's
chain -- ``hybrid_engine._sample`` (``.float()``, divide, ``topk``,
``masked_fill``, ``softmax``, ``multinomial``), with the sort-based HF nucleus
filter added for the ``top_p < 1`` case.  The two alternate call by call in
one process; each call is timed with device events and the median of
``--calls`` calls after a warm-up is reported.

Decode loop: per-token time of the hybrid engine's graph-replayed rollout
(the loop of ``scripts/bench_decode.py``) with the draw inside the captured
step (``fused_sampling=True``) and with the torch chain outside it.

Log-prob and entropy: forward + backward of ``ops.token_stats.token_logprobs
(with_entropy=True)`` on ``[B, R, V]`` bf16 logits sliced out of ``[B, 2R, V]``,
against the ``log_softmax`` expressions of ``rl/ppo_utils``.  Time (device
events, forward and backward apart), ``torch.cuda.max_memory_allocated`` as a
rise over the resident logits, and achieved bytes/s counted from the least
traffic: 2 B per logit forward, 4 B per logit backward.  These are rates of the
whole op, not of a kernel.

    python scripts/bench_rl_token_ops.py [--out profiles/r7/rl_token_ops_ab.jsonl]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from dlrover_wuqiong_amd.atorch.rl.hybrid_engine import HybridEngine, _sample  # noqa: E402
from dlrover_wuqiong_amd.ops.sampling import sample_tokens  # noqa: E402
from dlrover_wuqiong_amd.ops.token_stats import token_logprobs  # noqa: E402


def torch_chain(logits, temperature, top_k, top_p):
    """Today's sampling chain; for top_p < 1 the HF sort-based nucleus filter
    between top-k and the softmax."""
    if top_p >= 1.0:
        return _sample(logits.float(), temperature, top_k, None)
    z = logits.float() / temperature
    if top_k:
        kth = z.topk(top_k, dim=-1).values[:, -1:]
        z = z.masked_fill(z < kth, float("-inf"))
    zs, idx = z.sort(dim=-1, descending=False)
    cum = zs.softmax(-1).cumsum(-1)
    drop = cum <= 1.0 - top_p
    drop[:, -1:] = False
    z = z.masked_fill(drop.scatter(1, idx, drop), float("-inf"))
    return torch.multinomial(z.softmax(-1), 1)


def _timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3  # us


def bench_sampler(calls, emit):
    for B in (8, 64):
        for Vv in (32000, 128256):
            torch.manual_seed(0)
            logits = (3 * torch.randn(B, Vv, device="cuda")).to(torch.bfloat16)
            offset = torch.zeros(1, device="cuda", dtype=torch.int64)
            for top_k, top_p in ((50, 0.95), (0, 1.0)):
                fused = lambda: sample_tokens(logits, 1.0, top_k, top_p, seed=1, offset=offset)  # noqa: E731
                chain = lambda: torch_chain(logits, 1.0, top_k, top_p)  # noqa: E731
                for _ in range(20):
                    fused()
                    chain()
                torch.cuda.synchronize()
                tf, tc = [], []
                for _ in range(calls):
                    tf.append(_timed(fused))
                    tc.append(_timed(chain))
                emit({"bench": "sampler", "B": B, "V": Vv, "dtype": "bf16", "top_k": top_k, "top_p": top_p,
                      "calls": calls, "fused_us_median": round(statistics.median(tf), 1),
                      "fused_us_min": round(min(tf), 1), "torch_chain_us_median": round(statistics.median(tc), 1),
                      "torch_chain_us_min": round(min(tc), 1),
                      "speedup_median": round(statistics.median(tc) / statistics.median(tf), 2)})


def bench_decode(model, batch, prompt, new, emit):
    from dlrover_wuqiong_amd.models.llama import Llama, LlamaConfig

    torch.manual_seed(0)
    cfg = LlamaConfig.named(model)
    with torch.device("cuda"):
        m = Llama(cfg)
    m = m.to(torch.bfloat16).eval()
    p = torch.randint(0, cfg.vocab_size, (batch, prompt), device="cuda")
    eng = HybridEngine(m, batch, prompt + new, use_graph=True)
    kw = dict(temperature=1.0, top_k=50, top_p=0.95)
    runs = {True: [], False: []}
    for fused in (True, False):
        eng.generate(p, 8, fused_sampling=fused, seed=1, **kw)  # warm-up
    for _ in range(3):
        for fused in (True, False):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.generate(p, new, fused_sampling=fused, seed=1, **kw)
            torch.cuda.synchronize()
            runs[fused].append(1e3 * (time.perf_counter() - t0) / new)
    emit({"bench": "decode_loop", "model": model, "batch": batch, "prompt": prompt, "new": new, "top_k": 50,
          "top_p": 0.95, "in_graph_sampling_ms_per_token": [round(v, 3) for v in runs[True]],
          "torch_chain_ms_per_token": [round(v, 3) for v in runs[False]],
          "note": "host clock around generate (prefill included) / new tokens; 3 alternating runs each"})
    del eng, m
    torch.cuda.empty_cache()


def _torch_stats(resp, labels):
    lp = F.log_softmax(resp.float(), dim=-1)
    return lp.gather(-1, labels.unsqueeze(-1)).squeeze(-1), -(lp.exp() * lp).sum(-1)


def bench_logprob(B, R, Vv, iters, emit):
    torch.manual_seed(0)
    full = torch.empty(B, 2 * R, Vv, device="cuda", dtype=torch.bfloat16)
    for b in range(B):  # filled per batch row: no fp32 [B, 2R, V] temporary
        full[b] = (3 * torch.randn(2 * R, Vv, device="cuda")).to(torch.bfloat16)
    full.requires_grad_()
    labels = torch.randint(0, Vv, (B, R), device="cuda")
    g1 = torch.randn(B, R, device="cuda")
    n_logits = B * R * Vv
    res = {}
    for name, fn in (("fused", lambda x: token_logprobs(x, labels, with_entropy=True)),
                     ("torch", lambda x: _torch_stats(x, labels))):
        tf, tb, peak = [], [], 0
        for it in range(iters + 2):
            full.grad = None
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            out = {}

            def fwd():
                resp = full[:, R - 1:-1, :]
                logp, ent = fn(resp)
                out["obj"] = (g1 * logp).sum() - 0.01 * ent.sum()

            f = _timed(fwd)
            b = _timed(lambda: out["obj"].backward())
            if it >= 2:
                tf.append(f)
                tb.append(b)
                peak = max(peak, torch.cuda.max_memory_allocated() - base)
            del out
        res[name] = {"fwd_ms": round(statistics.median(tf) / 1e3, 3), "bwd_ms": round(statistics.median(tb) / 1e3, 3),
                     "peak_rise_GiB": round(peak / 2**30, 3),
                     "fwd_GBps_of_2B_per_logit": round(2 * n_logits / (statistics.median(tf) * 1e-6) / 1e9, 1),
                     "bwd_GBps_of_4B_per_logit": round(4 * n_logits / (statistics.median(tb) * 1e-6) / 1e9, 1)}
    emit({"bench": "logprob_entropy", "shape": [B, R, Vv], "sliced_from": [B, 2 * R, Vv], "dtype": "bf16",
          "iters": iters, "fused": res["fused"], "torch": res["torch"],
          "note": "bwd includes autograd's slice backward (zero-fill and copy into the [B, 2R, V] gradient) for both"})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/r7/rl_token_ops_ab.jsonl")
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--decode-model", default="llama3-8b", help="'' skips the decode loop")
    ap.add_argument("--logprob-shape", default="8,512,128256")
    ap.add_argument("--iters", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_rl_token_ops.py measures on a GPU; none found")
    rows = []

    def emit(r):
        rows.append(r)
        print(json.dumps(r), flush=True)

    bench_sampler(a.calls, emit)
    B, R, Vv = (int(v) for v in a.logprob_shape.split(","))
    bench_logprob(B, R, Vv, a.iters, emit)
    if a.decode_model:
        bench_decode(a.decode_model, 8, 128, 128, emit)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
