#!/usr/bin/env python
"""A/B of the flat AdamW update kernels on one GPU, no model: dw_adam_flat
(fp32 moments) against dw_qadam_flat (8- and 4-bit block-quantized moments)
on the same parameter / master / gradient buffers.

bf16 parameters and gradients with an fp32 master.  After a warm-up the
kernels alternate (one launch of each per repetition, not blocks of one
kernel); every launch is timed alone with device events; the figure is the
median.  One JSON line per (kernel, n): time, bytes moved (28 B/element for
fp32 moments, 16 + 1/16 at 8 bits, 14 + 1/16 at 4 bits), achieved TB/s and
the ratio to dw_adam_flat in the same run.

    python scripts/bench_qadam_flat.py --out profiles/r7/qadam_flat_ab.jsonl
"""

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dlrover_wuqiong_amd.ops import _hip  # noqa: E402

SIZES = {"gpt2-1.5b": 1_560_000_000, "1e9": 1_000_000_000, "llama3-8b/8": 1_003_750_016}
HP = dict(lr=1e-4, b1=0.9, b2=0.95, eps=1e-8, wd=0.1)
BYTES = {"fp32": 28.0, 8: 16.0 + 1.0 / 16, 4: 14.0 + 1.0 / 16}


def run_size(label, n, reps, warmup):
    dev = "cuda"
    L = _hip.lib()
    npad = (n + 127) // 128 * 128
    master = torch.randn(n, device=dev)
    param = master.to(torch.bfloat16)
    grad = (torch.randn(n, device=dev) * 0.01).to(torch.bfloat16)
    mask = (torch.rand(n // 64, device=dev) > 0.1).to(torch.uint8)
    gs = torch.full((1,), 0.5, device=dev)
    m = torch.zeros(n, device=dev)
    v = torch.zeros(n, device=dev)
    q = {b: [torch.zeros(npad * b // 8, dtype=torch.uint8, device=dev) for _ in range(2)]
         + [torch.zeros(npad // 128, device=dev) for _ in range(2)] for b in (8, 4)}
    step = [0]

    def bc():
        t = max(1, step[0])
        return 1 - HP["b1"] ** t, 1 - HP["b2"] ** t

    def adam():
        bc1, bc2 = bc()
        _hip.check(L.dw_adam_flat(_hip.ptr(param), 1, _hip.ptr(master), _hip.ptr(grad), 1, _hip.ptr(m), _hip.ptr(v),
                                  _hip.ptr(gs), n, 0, HP["lr"], HP["b1"], HP["b2"], HP["eps"], HP["wd"], bc1, bc2, 1,
                                  _hip.ptr(mask), _hip.stream()), "adam")

    def qadam(bits):
        def f():
            bc1, bc2 = bc()
            mq, vq, ms, vs = q[bits]
            _hip.check(L.dw_qadam_flat(
                _hip.ptr(param), 1, _hip.ptr(master), _hip.ptr(grad), 1, _hip.ptr(mq), _hip.ptr(vq), _hip.ptr(ms),
                _hip.ptr(vs), _hip.ptr(gs), n, 0, HP["lr"], HP["b1"], HP["b2"], HP["eps"], HP["wd"], bc1, bc2, 1,
                _hip.ptr(mask), bits, _hip.stream()), "qadam")
        return f

    # name -> (launch, moment format)
    kernels = {"adam_flat_fp32": (adam, "fp32"), "qadam_flat_8bit": (qadam(8), 8), "qadam_flat_4bit": (qadam(4), 4)}
    times = {k: [] for k in kernels}
    for r in range(warmup + reps):
        step[0] += 1
        for name, (launch, _fmt) in kernels.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            launch()
            e1.record()
            e1.synchronize()
            if r >= warmup:
                times[name].append(e0.elapsed_time(e1))
    assert bool(torch.isfinite(master).all())
    base = statistics.median(times["adam_flat_fp32"])
    rows = []
    for name, (_launch, fmt) in kernels.items():
        t = statistics.median(times[name])
        nbytes = BYTES[fmt] * n
        rows.append({"kernel": name, "size": label, "n": n, "moments": fmt,
                     "ms_median": round(t, 4), "ms_min": round(min(times[name]), 4),
                     "ms_max": round(max(times[name]), 4), "reps": reps, "bytes_per_element": round(BYTES[fmt], 4),
                     "bytes": int(nbytes), "tb_per_s": round(nbytes / (t * 1e-3) / 1e12, 3),
                     "ratio_to_adam_flat_fp32": round(t / base, 4),
                     "byte_ratio": round(BYTES[fmt] / BYTES["fp32"], 4)})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/r7/qadam_flat_ab.jsonl")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", default=",".join(SIZES), help="labels of SIZES, or element counts")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_qadam_flat: no GPU")
    if a.reps < 10:
        sys.exit("bench_qadam_flat: at least 10 repetitions")
    rows = []
    for s in a.sizes.split(","):
        label, n = (s, SIZES[s]) if s in SIZES else (s, int(float(s)))
        rows += run_size(label, n, a.reps, a.warmup)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for r in rows:
            line = json.dumps(r)
            print(line)
            f.write(line + "\n")


if __name__ == "__main__":
    main()
