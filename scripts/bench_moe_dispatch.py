"""MoE token path alone, fused kernels against the torch-op path.

One ``MoELayer`` per shape with the experts replaced by the identity, so a
step is: gate projection + router, expert sort, dispatch, combine, forward
and backward.  ``fused``: the layer's fused path (``ops/moe.py``: router,
sort, gather and k-way row-sum kernels).  ``unfused``: ``fused_dispatch=False``
with the router kernel switched off too, i.e. the chain of torch ops.  The
two are timed alternately in the same process (device events around ``iters``
steps, after a warm-up), ``repeats`` times each; the spread is the min / max
over the repeats.  The launches per step are counted in a separate, untimed
pass with the profiler.  Bytes: the rows the token path has to move,
(7 T k + 2 T) H 2 -- dispatch fwd reads and writes T k rows, combine fwd reads
T k and writes T, combine bwd reads dout and y and writes dy (3 T k), dispatch
bwd reads T k and writes T -- over the step time (a whole-path rate, not a
kernel's).

    python scripts/bench_moe_dispatch.py [--out profiles/moe_dispatch_ab.jsonl]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

from dlrover_wuqiong_amd.ops import moe as moe_ops  # noqa: E402
from dlrover_wuqiong_amd.parallel.moe import MoELayer  # noqa: E402

SHAPES = [(8192, 4096, 8, 2), (8192, 2048, 64, 6)]  # (T, H, E, k)


class _IdentityExperts(nn.Module):
    def forward(self, x, counts):
        return x


def _layer(H, E, k, fused):
    m = MoELayer(H, 8, num_experts=E, top_k=k, fused_dispatch=fused, dtype=torch.bfloat16, device="cuda")
    m.experts = _IdentityExperts()
    return m


class _TorchRouter:
    """Switch the router kernel off inside the block (the unfused baseline)."""

    def __enter__(self):
        self.saved = moe_ops.route_kernel_takes
        moe_ops.route_kernel_takes = lambda logits, k: False

    def __exit__(self, *a):
        moe_ops.route_kernel_takes = self.saved


def _step(m, x, go, fused):
    x.grad = None
    m.gate.wg.weight.grad = None
    if fused:
        y = m(x)
        (y.float().mul(go).sum() + m.aux_loss).backward()
    else:
        with _TorchRouter():
            y = m(x)
            (y.float().mul(go).sum() + m.aux_loss).backward()
    return y


def _time(m, x, go, fused, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        _step(m, x, go, fused)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def _launches(m, x, go, fused):
    from torch.profiler import ProfilerActivity, profile

    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        _step(m, x, go, fused)
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)


def run(T, H, E, k, iters, repeats):
    if not torch.cuda.is_available():
        raise SystemExit("bench_moe_dispatch: needs a GPU")
    torch.manual_seed(0)
    mf, mu = _layer(H, E, k, True), _layer(H, E, k, False)
    mu.load_state_dict(mf.state_dict())
    x = torch.randn(T, H, device="cuda").bfloat16().requires_grad_(True)
    go = torch.randn(T, H, device="cuda")
    for _ in range(5):
        yf = _step(mf, x, go, True).detach()
        gf = x.grad.clone()
        yu = _step(mu, x, go, False).detach()
        gu = x.grad.clone()
    torch.cuda.synchronize()
    tf, tu = [], []
    for _ in range(repeats):  # alternate the two
        tf.append(_time(mf, x, go, True, iters))
        tu.append(_time(mu, x, go, False, iters))
    nbytes = (7 * T * k + 2 * T) * H * 2
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    res = {
        "T": T, "H": H, "E": E, "k": k, "iters": iters, "repeats": repeats,
        "fused_ms": round(med(tf), 4), "fused_ms_min_max": [round(min(tf), 4), round(max(tf), 4)],
        "unfused_ms": round(med(tu), 4), "unfused_ms_min_max": [round(min(tu), 4), round(max(tu), 4)],
        "speedup": round(med(tu) / med(tf), 3),
        # faster by more than the run-to-run spread: the slowest fused repeat beats the fastest unfused one
        "fused_faster_beyond_spread": max(tf) < min(tu),
        "fused_tbs": round(nbytes / (med(tf) * 1e-3) / 1e12, 3),
        "unfused_tbs": round(nbytes / (med(tu) * 1e-3) / 1e12, 3),
        "out_rel_diff": float((yf.float() - yu.float()).norm() / yu.float().norm()),
        "dx_rel_diff": float((gf.float() - gu.float()).norm() / gu.float().norm()),
    }
    try:
        res["fused_launches"] = _launches(mf, x, go, True)
        res["unfused_launches"] = _launches(mu, x, go, False)
    except Exception as e:  # the profiler is optional equipment; the timings stand without it
        res["launches_error"] = repr(e)[:200]
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "moe_dispatch_ab.jsonl"))
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for T, H, E, k in SHAPES:
            line = json.dumps(run(T, H, E, k, a.iters, a.repeats))
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
