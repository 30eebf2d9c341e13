"""The decode step's GEMMs through the weight-streaming kernel (1 GPU):
what ``HybridEngine(rollout_weights=...)`` is worth (docs/rl_fp8_rollouts.md).

``--part shapes``: per GEMM shape of Llama-3 8B and ``M`` in {1, 8, 16, 64}:
``F.linear`` (hipBLASLt, what the decode step runs without the option), the
skinny kernel on bf16 weights and on e4m3 weights, alternating in one process.
Each variant is a captured graph of R launches over R different weight
buffers (at least 1 GB of e4m3, 2 GB of bf16: a weight is read once per
token, never from a cache the previous replay filled), timed with device
events around ``--iters`` replays (40: a window of 15 - 60 ms).  GB/s counts the weight bytes only.

``--part rollout``: ms per token of ``generate_ragged`` (Llama-3 8B, B = 8,
128 + 128 tokens, graph decode, fused sampling, ``fused_kv_append`` on; the
method of ``scripts/bench_rl_ragged_rollout.py``) for four engines
alternating: built as before this option existed (no keyword), with
``rollout_weights=None``, ``"bf16"`` and ``"fp8"``.

``--part distance``: mean / max over response tokens of
``|logp_bf16 - logp_fp8|`` for an ``"fp8"`` rollout: ``logp_bf16`` from the
model's full forward over the sequences, ``logp_fp8`` from teacher-forcing the
same tokens through the e4m3 decode path.

``--part sweep``: the layer shapes with ``splits`` forced to 1 .. 16, the data
behind the kernel's own choice of the K split.

    python scripts/bench_rl_decode_gemm.py [--part all] [--out profiles/r8/rl_decode_gemm_ab.jsonl]
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

from dlrover_wuqiong_amd.atorch.rl.hybrid_engine import HybridEngine  # noqa: E402
from dlrover_wuqiong_amd.models.llama import Llama, LlamaConfig  # noqa: E402
from dlrover_wuqiong_amd.ops.skinny_gemm import quantize_rows_e4m3, skinny_linear  # noqa: E402

# N x K of Llama-3 8B: qkv, o, gate|up, down, LM head
SHAPES = [("qkv_proj", 6144, 4096), ("o_proj", 4096, 4096), ("gate_up_proj", 28672, 4096),
          ("down_proj", 4096, 14336), ("lm_head", 128256, 4096)]
ROWS = [1, 8, 16, 64]


def _summary(v, nd=3):
    return {"median": round(statistics.median(v), nd), "min": round(min(v), nd), "max": round(max(v), nd)}


def _graph_of(fn, n):
    """A captured graph of fn(0) .. fn(n - 1), after one eager pass (warm-up,
    workspaces)."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        for i in range(n):
            fn(i)
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            keep = [fn(i) for i in range(n)]
    torch.cuda.current_stream().wait_stream(s)
    return g, keep


def _time_graph(g, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        g.replay()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def part_shapes(a, emit):
    for name, N, K in SHAPES:
        R = max(2, -(-(1 << 30) // (N * K)))
        gen = torch.Generator(device="cuda").manual_seed(N + K)
        wb = [(torch.randn(N, K, device="cuda", generator=gen) * 0.02).to(torch.bfloat16) for _ in range(R)]
        wq = [quantize_rows_e4m3(w) for w in wb]
        for M in ROWS:
            x = torch.randn(M, K, device="cuda", generator=gen).to(torch.bfloat16)
            variants = {
                "f_linear": lambda i: F.linear(x, wb[i]),
                "skinny_bf16": lambda i: skinny_linear(x, wb[i]),
                "skinny_fp8": lambda i: skinny_linear(x, wq[i][0], wq[i][1]),
            }
            graphs = {k: _graph_of(fn, R) for k, fn in variants.items()}
            for g, _ in graphs.values():
                _time_graph(g, 1)
            us = {k: [] for k in variants}
            for _ in range(a.runs):
                for k, (g, _) in graphs.items():
                    us[k].append(1e3 * _time_graph(g, a.iters) / (a.iters * R))
            nbytes = {"f_linear": 2 * N * K, "skinny_bf16": 2 * N * K, "skinny_fp8": N * K}
            ref = graphs["f_linear"][1][0].float()
            row = {"bench": "decode_gemm", "gemm": name, "N": N, "K": K, "M": M, "weight_buffers": R,
                   "iters": a.iters, "runs": a.runs,
                   "us": {k: _summary(v) for k, v in us.items()},
                   "weight_GBps": {k: {s: round(nbytes[k] / (1e3 * t), 1) for s, t in
                                       (("median", statistics.median(v)), ("at_min_us", min(v)),
                                        ("at_max_us", max(v)))} for k, v in us.items()},
                   "max_abs_diff_vs_f_linear": {k: round(float((graphs[k][1][0].float() - ref).abs().max()), 5)
                                                for k in ("skinny_bf16", "skinny_fp8")},
                   "ref_abs_max": round(float(ref.abs().max()), 4),
                   "note": "device events around graph replays; every launch of a replay reads another weight buffer"}
            emit(row)
            del graphs
        del wb, wq
        torch.cuda.empty_cache()


def part_sweep(a, emit):
    """The K split: every layer shape at M = 8 and 64, both weight forms,
    ``splits`` forced to 1 .. 16 (the data behind dw_skinny_gemm_splits)."""
    from dlrover_wuqiong_amd.ops import _hip

    for name, N, K in SHAPES[:4]:
        R = max(2, -(-(1 << 30) // (N * K)))
        gen = torch.Generator(device="cuda").manual_seed(1)
        wb = [(torch.randn(N, K, device="cuda", generator=gen) * 0.02).to(torch.bfloat16) for _ in range(R)]
        wq = [quantize_rows_e4m3(w) for w in wb]
        for M in (8, 64):
            x = torch.randn(M, K, device="cuda", generator=gen).to(torch.bfloat16)
            res = {}
            for form in ("bf16", "fp8"):
                for s in (1, 2, 3, 4, 6, 8, 12, 16):
                    if form == "bf16":
                        g, _ = _graph_of(lambda i: skinny_linear(x, wb[i], splits=s), R)
                    else:
                        g, _ = _graph_of(lambda i: skinny_linear(x, wq[i][0], wq[i][1], splits=s), R)
                    _time_graph(g, 1)
                    t = [1e3 * _time_graph(g, a.iters) / (a.iters * R) for _ in range(a.runs)]
                    res[f"{form}/{s}"] = _summary(t, 2)
            emit({"bench": "split_sweep", "gemm": name, "N": N, "K": K, "M": M, "weight_buffers": R,
                  "iters": a.iters, "runs": a.runs, "auto": int(_hip.lib().dw_skinny_gemm_splits(M, N, K)),
                  "us": res, "note": "'auto' is the kernel's own choice; same method as the decode_gemm rows"})
        del wb, wq
        torch.cuda.empty_cache()


def _model(name):
    torch.manual_seed(0)
    cfg = LlamaConfig.named(name)
    with torch.device("cuda"):
        m = Llama(cfg)
    return m.to(torch.bfloat16).eval()


def _clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), out


def part_rollout(a, emit, m):
    cfg = m.cfg
    B, P, T = a.batch, a.prompt, a.new
    p = torch.randint(0, cfg.vocab_size, (B, P), device="cuda")
    full = torch.full((B,), P, device="cuda")
    kw = dict(temperature=1.0, top_k=50, top_p=0.95, fused_sampling=True, seed=1)
    engines = {
        "as_before_the_option": HybridEngine(m, B, P + T, use_graph=True, fused_kv_append=True),
        "unset": HybridEngine(m, B, P + T, use_graph=True, fused_kv_append=True, rollout_weights=None),
        "bf16": HybridEngine(m, B, P + T, use_graph=True, fused_kv_append=True, rollout_weights="bf16"),
        "fp8": HybridEngine(m, B, P + T, use_graph=True, fused_kv_append=True, rollout_weights="fp8"),
    }
    for e in engines.values():
        e.generate_ragged(p, full, 8, **kw)  # warm-up
    ms, seqs = {k: [] for k in engines}, {}
    for _ in range(a.runs):
        for k, e in engines.items():
            t, out = _clock(lambda: e.generate_ragged(p, full, T, **kw))
            seqs[k] = out[0]
            ms[k].append(t / T)
    emit({"bench": "rollout_ms_per_token", "model": a.model, "batch": B, "prompt": P, "new": T, "top_k": 50,
          "top_p": 0.95, "graph": True, "fused_sampling": True, "fused_kv_append": True, "runs": a.runs,
          "ms_per_token": {k: dict(_summary(v), runs=[round(x, 3) for x in v]) for k, v in ms.items()},
          "same_tokens_unset_vs_before": bool(torch.equal(seqs["unset"], seqs["as_before_the_option"])),
          "same_tokens_bf16_vs_before": bool(torch.equal(seqs["bf16"], seqs["as_before_the_option"])),
          "note": "host clock around generate_ragged (prefill, fp8 requantisation and capture included) / new "
                  "tokens; alternating runs; 'as_before_the_option' and 'unset' run the same code"})


@torch.no_grad()
def part_distance(a, emit, m, name):
    cfg = m.cfg
    B, P, T = a.batch, min(a.prompt, cfg.max_position_embeddings // 4), min(a.new, cfg.max_position_embeddings // 4)
    p = torch.randint(0, cfg.vocab_size, (B, P), device="cuda")
    eng = HybridEngine(m, B, P + T, use_graph=False, fused_kv_append=True, rollout_weights="fp8")
    seq = eng.generate(p, T, temperature=1.0, top_k=50, top_p=0.95, fused_sampling=True, seed=3)
    resp = seq[:, P:]
    # bf16 policy: the full forward that make_experience scores with
    lp_bf16 = torch.log_softmax(m(seq[:, :-1])[:, P - 1:].float(), -1).gather(-1, resp[..., None])[..., 0]
    # fp8 policy: the same tokens teacher-forced through the decode path
    eng._ensure_cache(B, p.device, torch.bfloat16)
    eng._refresh_rollout_weights()
    logits = [eng._forward(p, prefill=True)]
    for t in range(T - 1):
        logits.append(eng._forward(resp[:, t:t + 1], prefill=False).clone())
    lp_fp8 = torch.log_softmax(torch.stack(logits, 1).float(), -1).gather(-1, resp[..., None])[..., 0]
    # the first response token comes from the bf16 prefill in both: leave it out
    d = (lp_bf16 - lp_fp8).abs()[:, 1:]
    # the same comparison for the bf16 decode path: what prefill-vs-decode kernels differ by on their own
    eb = HybridEngine(m, B, P + T, use_graph=False, fused_kv_append=True, rollout_weights="bf16")
    eb._ensure_cache(B, p.device, torch.bfloat16)
    logits = [eb._forward(p, prefill=True)]
    for t in range(T - 1):
        logits.append(eb._forward(resp[:, t:t + 1], prefill=False).clone())
    lp_dec = torch.log_softmax(torch.stack(logits, 1).float(), -1).gather(-1, resp[..., None])[..., 0]
    d0 = (lp_bf16 - lp_dec).abs()[:, 1:]
    emit({"bench": "fp8_policy_distance", "model": name, "weights": "random init", "batch": B, "prompt": P,
          "response_tokens": int(d.numel()), "abs_logp_diff_fp8_decode_vs_bf16_forward":
              {"mean": round(float(d.mean()), 5), "max": round(float(d.max()), 5)},
          "abs_logp_diff_bf16_decode_vs_bf16_forward":
              {"mean": round(float(d0.mean()), 5), "max": round(float(d0.max()), 5)},
          "mean_logp_bf16": round(float(lp_bf16.mean()), 4),
          "note": "sampled with top_k 50 / top_p 0.95 from the fp8 engine; log-probs over the full vocabulary"})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/r8/rl_decode_gemm_ab.jsonl")
    ap.add_argument("--part", default="all", choices=["all", "shapes", "sweep", "rollout", "distance"])
    ap.add_argument("--model", default="llama3-8b")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--prompt", type=int, default=128)
    ap.add_argument("--new", type=int, default=128)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--iters", type=int, default=40, help="graph replays per timed window (tens of ms)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_rl_decode_gemm.py measures on a GPU; none found")
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    f = open(a.out, "w")

    def emit(r):
        line = json.dumps(r)
        print(line, flush=True)
        f.write(line + "\n")
        f.flush()

    if a.part in ("all", "shapes"):
        part_shapes(a, emit)
    if a.part in ("all", "sweep"):
        part_sweep(a, emit)
    if a.part in ("all", "distance"):
        part_distance(a, emit, _model("llama-tiny"), "llama-tiny")
    if a.part in ("all", "rollout") or (a.part == "distance" and a.model != "llama-tiny"):
        m = _model(a.model)
        if a.part in ("all", "rollout"):
            part_rollout(a, emit, m)
        if a.part in ("all", "distance") and a.model != "llama-tiny":
            part_distance(a, emit, m, a.model)
    f.close()


if __name__ == "__main__":
    main()
