"""The expert FFN of an MoE decode step through the weight-streaming kernels
(1 GPU): what ``HybridEngine(moe_experts=...)`` is worth (docs/rl_moe_decode.md).

``--part op``: per layer shape (Mixtral-8x7B: E=8, k=2, H=4096, F=14336; a
fine-grained layer: E=64, k=6, H=2048, F=1408) and ``T`` in {1, 8, 16, 64}:
the module's own path (``MoELayer.forward``: gate, router, sort, dispatch,
grouped GEMMs, SwiGLU, combine) against ``mlp.gate`` + ``moe_stream_mlp`` on the
bf16 weights and on e4m3 copies, alternating in one process, eager (device
events around ``--iters`` passes over the layers) and as a captured graph of
one call per layer.  ``--layers`` layers with their own weights and their own
tokens take turns, so that a replay never finds its experts in a cache the
previous one filled.  GB/s counts the weight bytes of the experts the router
actually picked.

``--part engine``: ms per token of ``generate_ragged`` for a Mixtral-8x7B
actor cut to ``--model-layers`` layers (B = 8, 128 + 64 tokens, greedy) with
the option unset (eager decode, the module's path), ``"bf16"`` and ``"fp8"``
(both captured), alternating.

    python scripts/bench_rl_decode_moe.py [--part all] [--out profiles/rl_moe_decode.jsonl]
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
from dlrover_wuqiong_amd.ops.moe_stream import moe_stream_mlp, workspace_bytes  # noqa: E402
from dlrover_wuqiong_amd.ops.skinny_gemm import quantize_rows_e4m3  # noqa: E402
from dlrover_wuqiong_amd.parallel.moe import MoELayer  # noqa: E402

LAYERS = {"mixtral-8x7b": dict(E=8, k=2, H=4096, F=14336), "fine-grained": dict(E=64, k=6, H=2048, F=1408)}
ROWS = [1, 8, 16, 64]


def _summary(v, nd=3):
    return {"median": round(statistics.median(v), nd), "min": round(min(v), nd), "max": round(max(v), nd)}


def _events(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def _graph_of(fn):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        fn()
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            keep = fn()
    torch.cuda.current_stream().wait_stream(s)
    return g, keep


@torch.no_grad()
def part_op(a, emit):
    for name, d in LAYERS.items():
        E, k, H, F = d["E"], d["k"], d["H"], d["F"]
        torch.manual_seed(E + F)
        mlps = [MoELayer(H, F, E, k, dtype=torch.bfloat16, device="cuda").eval() for _ in range(a.layers)]
        fp8 = []
        for m in mlps:
            q = [quantize_rows_e4m3(p.detach().view(-1, p.shape[2])) for p in (m.experts.w1, m.experts.w3, m.experts.w2)]
            fp8.append((tuple(c.view(p.shape) for (c, _), p in zip(q, (m.experts.w1, m.experts.w3, m.experts.w2))),
                        tuple(s.view(E, -1) for _, s in q)))
        for T in ROWS:
            xs = [torch.randn(T, H, device="cuda").to(torch.bfloat16) for _ in mlps]
            ws = torch.empty(workspace_bytes(T, k, E, H, F), device="cuda", dtype=torch.uint8)
            routed = sum(int(m.gate(x)[1].unique().numel()) for m, x in zip(mlps, xs)) / len(mlps)

            def stream(i, form):
                m = mlps[i]
                w, idx, _ = m.gate(xs[i])
                if form == "fp8":
                    return moe_stream_mlp(xs[i], w, idx, *fp8[i][0], scales=fp8[i][1], workspace=ws)
                return moe_stream_mlp(xs[i], w, idx, m.experts.w1, m.experts.w3, m.experts.w2, workspace=ws)

            variants = {"module": lambda: [m(x) for m, x in zip(mlps, xs)],
                        "stream_bf16": lambda: [stream(i, "bf16") for i in range(len(mlps))],
                        "stream_fp8": lambda: [stream(i, "fp8") for i in range(len(mlps))]}
            graphs, failed = {}, {}
            for key, fn in variants.items():
                fn()   # warm-up
                try:
                    graphs[key] = _graph_of(fn)[0]
                    graphs[key].replay()
                except Exception as e:   # the module's path may read the host
                    failed[key] = f"{type(e).__name__}: {str(e)[:200]}"
            torch.cuda.synchronize()
            us = {f"{key}/{mode}": [] for key in variants for mode in ("eager", "graph")
                  if mode == "eager" or key in graphs}
            for _ in range(a.runs):
                for key, fn in variants.items():
                    us[f"{key}/eager"].append(1e3 * _events(fn, a.iters) / len(mlps))
                    if key in graphs:
                        us[f"{key}/graph"].append(1e3 * _events(graphs[key].replay, a.iters) / len(mlps))
            nbytes = {key: routed * 3 * F * H * (1 if "fp8" in key else 2) for key in us}
            ref = mlps[0](xs[0]).float()
            emit({"bench": "moe_decode_op", "layer": name, **d, "T": T, "layers_alternating": len(mlps),
                  "iters": a.iters, "runs": a.runs, "routed_experts_per_layer": routed,
                  "us_per_layer": {key: _summary(v, 2) for key, v in us.items()},
                  "routed_weight_GBps": {key: round(nbytes[key] / (1e3 * statistics.median(v)), 1)
                                         for key, v in us.items()},
                  "capture_failed": failed,
                  "max_abs_diff_vs_module": {f: round(float((stream(0, f).float() - ref).abs().max()), 5)
                                             for f in ("bf16", "fp8")},
                  "ref_abs_max": round(float(ref.abs().max()), 4),
                  "note": "device events; the gate GEMM and the router are inside every variant"})
        del mlps, fp8
        torch.cuda.empty_cache()


def _clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), out


def part_engine(a, emit):
    cfg = LlamaConfig.named("mixtral-8x7b")
    cfg.num_hidden_layers = a.model_layers
    torch.manual_seed(0)
    torch.set_default_dtype(torch.bfloat16)   # 2.8 GB of experts per layer: never hold them in fp32
    with torch.device("cuda"):
        m = Llama(cfg).eval()
    torch.set_default_dtype(torch.float32)
    B, P, T = a.batch, a.prompt, a.new
    p = torch.randint(0, cfg.vocab_size, (B, P), device="cuda")
    full = torch.full((B,), P, device="cuda")
    engines = {mode or "unset": HybridEngine(m, B, P + T, use_graph=True, moe_experts=mode)
               for mode in (None, "bf16", "fp8")}
    for e in engines.values():
        e.generate_ragged(p, full, 4, temperature=0)   # warm-up
    ms, seqs = {key: [] for key in engines}, {}
    for _ in range(a.runs):
        for key, e in engines.items():
            t, out = _clock(lambda: e.generate_ragged(p, full, T, temperature=0))
            seqs[key] = out[0]
            ms[key].append(t / T)
    emit({"bench": "moe_rollout_ms_per_token", "model": "mixtral-8x7b", "layers": a.model_layers, "batch": B,
          "prompt": P, "new": T, "greedy": True, "runs": a.runs,
          "graph": {key: e.use_graph for key, e in engines.items()},
          "ms_per_token": {key: dict(_summary(v), runs=[round(x, 3) for x in v]) for key, v in ms.items()},
          "same_tokens_bf16_vs_unset": bool(torch.equal(seqs["bf16"], seqs["unset"])),
          "note": "host clock around generate_ragged (prefill, e4m3 requantisation and capture included) / new "
                  "tokens; alternating runs; random-init weights"})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/rl_moe_decode.jsonl")
    ap.add_argument("--part", default="all", choices=["all", "op", "engine"])
    ap.add_argument("--layers", type=int, default=4, help="layers that take turns in --part op")
    ap.add_argument("--model-layers", type=int, default=8, help="Mixtral layers of the --part engine actor")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--prompt", type=int, default=128)
    ap.add_argument("--new", type=int, default=64)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50, help="passes per timed window")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_rl_decode_moe.py measures on a GPU; none found")
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        def emit(r):
            line = json.dumps(r)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()

        if a.part in ("all", "op"):
            part_op(a, emit)
        if a.part in ("all", "engine"):
            part_engine(a, emit)


if __name__ == "__main__":
    main()
