"""Expert FFN alone: fused SwiGLU gate/up launch against the unfused chain.

A step is ``grouped_mlp`` forward + backward over fixed per-expert counts (no
router, no dispatch).  ``fused``: ``fused_glu=True`` -- gate, up and the
activation in one grouped launch, dual-weight dgrad
(``ops.grouped_gemm.grouped_swiglu_linear``).  ``unfused``: ``fused_glu=False``
-- two grouped GEMMs, ``silu`` and ``mul`` as torch ops, two dgrad GEMMs and
an add.  The two are timed alternately in the same process (device events
around ``iters`` steps, after a warm-up), ``repeats`` times each; the spread
is the min / max over the repeats.  Launches per step are counted in a
separate, untimed pass with the profiler.  Memory, both as a rise over the
resident tensors (inputs, weights, ``go``): ``held`` is what is allocated
between the forward and the backward (the output and what autograd saved),
``peak`` is ``torch.cuda.max_memory_allocated`` over one whole step (it falls
in the backward, where the three weight gradients are allocated too).
FLOP/s: the 9 GEMMs of a step (3 forward, 6 backward), 2 n H F each, over the
step time (a whole-path rate, not a kernel's).

Shapes are ones ``grouped_mlp`` sends to the grouped kernel (many small
experts), each with balanced counts and with a skewed split that leaves
every eighth expert empty.

    python scripts/bench_moe_experts.py [--out profiles/moe_experts_ab.jsonl]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from dlrover_wuqiong_amd.parallel.moe import grouped_mlp  # noqa: E402

SHAPES = [(49152, 2048, 1408, 64), (32768, 4096, 2048, 128)]  # (n, H, F, E)


def make_counts(n, E, split):
    if split == "balanced":
        c = [n // E] * E
    else:  # every eighth expert empty, the rest 1 : 2 : ... : 7 repeating
        w = [(e % 8) for e in range(E)]
        c = [n * v // sum(w) for v in w]
    c[-1] += n - sum(c)
    assert sum(c) == n and min(c) >= 0
    return c


def _step(x, counts, w1, w2, w3, go, fused):
    for t in (x, w1, w2, w3):
        t.grad = None
    y = grouped_mlp(x, counts, w1, w2, w3, "silu", fused_glu=fused)
    y.backward(go)
    return y


def _time(args, fused, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        _step(*args, fused)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def _memory(args, fused):
    """(held between forward and backward, peak over the step), bytes over the resident tensors."""
    x, counts, w1, w2, w3, go = args
    for t in (x, w1, w2, w3):
        t.grad = None
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    y = grouped_mlp(x, counts, w1, w2, w3, "silu", fused_glu=fused)
    torch.cuda.synchronize()
    held = torch.cuda.memory_allocated() - base
    y.backward(go)
    del y
    torch.cuda.synchronize()
    return held, torch.cuda.max_memory_allocated() - base


def _launches(args, fused):
    from torch.profiler import ProfilerActivity, profile

    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        _step(*args, fused)
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)


def run(n, H, F, E, split, iters, repeats):
    if not torch.cuda.is_available():
        raise SystemExit("bench_moe_experts: needs a GPU")
    assert not (E <= 16 and n >= 2048 * E), "shape would take the per-expert hipBLASLt path"
    torch.manual_seed(0)
    dev = "cuda"
    x = torch.randn(n, H, device=dev).bfloat16().requires_grad_(True)
    w1, w3 = ((torch.randn(E, F, H, device=dev) / H ** 0.5).bfloat16().requires_grad_(True) for _ in range(2))
    w2 = (torch.randn(E, H, F, device=dev) / F ** 0.5).bfloat16().requires_grad_(True)
    go = torch.randn(n, H, device=dev).bfloat16()
    counts = torch.tensor(make_counts(n, E, split), device=dev)
    args = (x, counts, w1, w2, w3, go)
    for _ in range(5):
        yf = _step(*args, True).detach()
        gf, g1f = x.grad.clone(), w1.grad.clone()
        yu = _step(*args, False).detach()
        gu, g1u = x.grad.clone(), w1.grad.clone()
    torch.cuda.synchronize()
    rel = lambda a, b: float((a.float() - b.float()).norm() / b.float().norm())  # noqa: E731
    diffs = {"out_rel_diff": rel(yf, yu), "dx_rel_diff": rel(gf, gu), "dw1_rel_diff": rel(g1f, g1u)}
    del yf, yu, gf, gu, g1f, g1u
    tf, tu = [], []
    for _ in range(repeats):  # alternate the two
        tf.append(_time(args, True, iters))
        tu.append(_time(args, False, iters))
    flops = 9 * 2 * n * H * F
    (held_f, peak_f), (held_u, peak_u) = _memory(args, True), _memory(args, False)
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    res = {
        "n": n, "H": H, "F": F, "E": E, "split": split, "empty_experts": int((counts == 0).sum()),
        "iters": iters, "repeats": repeats,
        "fused_ms": round(med(tf), 4), "fused_ms_min_max": [round(min(tf), 4), round(max(tf), 4)],
        "unfused_ms": round(med(tu), 4), "unfused_ms_min_max": [round(min(tu), 4), round(max(tu), 4)],
        "speedup": round(med(tu) / med(tf), 3),
        # faster by more than the run-to-run spread: the slowest fused repeat beats the fastest unfused one
        "fused_faster_beyond_spread": max(tf) < min(tu),
        "fused_tflops": round(flops / (med(tf) * 1e-3) / 1e12, 1),
        "unfused_tflops": round(flops / (med(tu) * 1e-3) / 1e12, 1),
        "fused_held_mib": round(held_f / 2 ** 20, 1), "unfused_held_mib": round(held_u / 2 ** 20, 1),
        "fused_peak_step_mib": round(peak_f / 2 ** 20, 1), "unfused_peak_step_mib": round(peak_u / 2 ** 20, 1),
        **diffs,
    }
    try:
        res["fused_launches"] = _launches(args, True)
        res["unfused_launches"] = _launches(args, False)
    except Exception as e:  # the profiler is optional equipment; the timings stand without it
        res["launches_error"] = repr(e)[:200]
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "moe_experts_ab.jsonl"))
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for n, H, F, E in SHAPES:
            for split in ("balanced", "skewed"):
                line = json.dumps(run(n, H, F, E, split, a.iters, a.repeats))
                print(line, flush=True)
                f.write(line + "\n")
                f.flush()
                torch.cuda.empty_cache()
