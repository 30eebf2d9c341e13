"""Fused LM head + token statistics against the path it replaces (1 GPU).

``ops.token_stats.linear_token_logprobs`` (csrc/kernels/linear_logprob.hip:
no logits) against ``token_logprobs(F.linear(X, W), labels, True)`` (hipBLASLt
GEMM that writes the bf16 ``[rows, V]`` logits, then the statistics kernel
that reads them back), no-grad, bf16, ``X ~ N(0, 1)``, ``W ~ N(0, 1) * 3 /
sqrt(H)``.  The two alternate call by call in one process; each call is timed
with device events and the median of ``--calls`` calls after a warm-up is
reported, with the rise of ``torch.cuda.max_memory_allocated`` over the
resident operands across one call.  ``fused_TFps`` counts 2 * rows * V * H
over the time of the whole fused op (both launches): a rate of the op, an
under-estimate of the main loop's.

    python scripts/bench_linear_logprob.py [--out profiles/linear_logprob_bench.jsonl]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from dlrover_wuqiong_amd.ops.token_stats import (linear_logprob_splits, linear_token_logprobs,  # noqa: E402
                                                 token_logprobs)


def _timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)  # ms


def _peak_rise(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


@torch.no_grad()
def bench(rows, H, V, calls, warmup):
    torch.manual_seed(0)
    X = torch.randn(rows, H, device="cuda").bfloat16()
    W = torch.empty(V, H, device="cuda", dtype=torch.bfloat16)
    for i in range(0, V, 8192):  # filled in pieces: no fp32 [V, H] temporary
        W[i:i + 8192] = (torch.randn(min(8192, V - i), H, device="cuda") * 3 / H ** 0.5).bfloat16()
    labels = torch.randint(0, V, (rows,), device="cuda")
    fused = lambda: linear_token_logprobs(X, W, labels, True)  # noqa: E731
    parent = lambda: token_logprobs(F.linear(X, W), labels, True)  # noqa: E731
    for _ in range(warmup):
        a = fused()
        b = parent()
    diff = max(float((x - y).abs().max()) for x, y in zip(a, b))
    del a, b
    tf, tp = [], []
    for _ in range(calls):
        tf.append(_timed(fused))
        tp.append(_timed(parent))
    mf, mp = statistics.median(tf), statistics.median(tp)
    return {"bench": "linear_logprob", "rows": rows, "H": H, "V": V, "dtype": "bf16", "calls": calls,
            "splits": linear_logprob_splits(rows, V), "fused_ms_median": round(mf, 3), "fused_ms_min": round(min(tf), 3),
            "parent_ms_median": round(mp, 3), "parent_ms_min": round(min(tp), 3),
            "parent_over_fused": round(mp / mf, 3), "fused_TFps": round(2.0 * rows * V * H / (mf * 1e-3) / 1e12, 1),
            "parent_TFps": round(2.0 * rows * V * H / (mp * 1e-3) / 1e12, 1),
            "fused_peak_rise_MiB": round(_peak_rise(fused) / 2**20, 2),
            "parent_peak_rise_MiB": round(_peak_rise(parent) / 2**20, 2),
            "max_abs_diff_fused_vs_parent": diff}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/linear_logprob_bench.jsonl")
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rows", default="4096,16384")
    ap.add_argument("--shapes", default="4096x128256,4096x32000", help="HxV,...")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_linear_logprob.py measures on a GPU; none found")
    out = []
    for hv in a.shapes.split(","):
        H, V = (int(v) for v in hv.split("x"))
        for rows in (int(v) for v in a.rows.split(",")):
            out.append(bench(rows, H, V, a.calls, a.warmup))
            print(json.dumps(out[-1]), flush=True)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        for r in out:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
