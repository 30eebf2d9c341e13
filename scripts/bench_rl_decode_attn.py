"""Decode attention over a bf16 against an e4m3 KV cache (1 GPU): what
``HybridEngine(kv_cache="fp8")`` (docs/rl_fp8_kv_cache.md) and
``HybridEngine(decode_kernel="mfma")`` (docs/rl_mfma_decode.md) are worth.

``--part kernel``: ``decode_attention`` on a bf16 cache (``bf16``:
``dw_attn_decode``, the VALU kernel, untouched; ``bf16_mfma``: the MFMA pass 1
``dw_attn_decode_mfma`` on the same buffers) against the e4m3 form (``fp8``:
``dw_attn_decode_q8``), alternating in one process: (H, Hkv, D) = (32, 8, 128)
and (64, 8, 128), B in {8, 64}, every row at len in {1024, 8192, 32768} where
the memory allows, per ``--chunks`` value.  Each variant is a captured graph
of R launches over R different cache buffers (>= ``--min-gb`` of e4m3 bytes in
all, so no launch finds its cache in L2 or the memory-side cache), device
events around the replays, time per launch; median and (min - max) of
``--runs``.  GB/s counts the cache bytes the launch reads (codes and scales).

``--part rollout``: ms per token of ``generate_ragged`` (Llama-3 8B, B = 8,
graph decode, fused sampling, ``fused_kv_append`` on, top_k 50 / top_p 0.95: the
configuration of the 5.68 ms row of docs/rl_ragged_rollouts.md) with a long
prompt, ``kv_cache`` unset and ``"fp8"`` and ``decode_kernel="mfma"`` (bf16
cache) alternating.  Host clock around the
call; the prefill of a long prompt dominates it, so the row also holds the
decode-only figure (t(new) - t(8)) / (new - 8).

``--part distance``: the policy-distance row of docs/rl_fp8_rollouts.md section
3 for the e4m3 cache (bf16 weights).

``--part shared`` (docs/rl_shared_prefix.md; not part of ``all``):
``decode_attention_shared`` over a prefix cache [Bp, P] and a suffix cache
[Bp * n, 512] (every row full) against ``decode_attention(kernel="mfma")`` on
the repeated [Bp * n, P + 512] cache with the same keys: (H, Hkv, D) =
(32, 8, 128), Bp = 8, n in {1, 4, 8, 16}, P in {1024, 8192}, per ``--chunks``
value; graphs, clock and summary as in ``--part kernel`` (R is sized so that the
shared form, the smaller one, walks through ``--min-gb`` per replay).  Then the
rollout row: ``generate_ragged`` of ``--batch`` prompts x ``--samples`` samples
with ``samples_per_prompt`` against the prompts repeated in the batch, both
with ``decode_kernel="mfma"`` and the unfused append.

One JSON line per row to ``--out``.
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
from dlrover_wuqiong_amd.ops.attention import decode_attention, decode_attention_shared  # noqa: E402
from dlrover_wuqiong_amd.ops.skinny_gemm import quantize_rows_e4m3  # noqa: E402

HEADS = [(32, 8, 128), (64, 8, 128)]
BATCHES = [8, 64]
LENS = [1024, 8192, 32768]


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


def part_kernel(a, emit):
    free = torch.cuda.mem_get_info()[0]
    for H, HKV, D in HEADS:
        for B in BATCHES:
            for n in LENS:
                row_bytes = B * n * HKV * D * 2            # K and V codes of one e4m3 cache
                R = max(2, -(-int(a.min_gb * 2 ** 30) // row_bytes))
                if R * row_bytes * 3.2 > 0.8 * free:       # bf16 + e4m3 buffers + scales
                    emit({"bench": "decode_attn", "H": H, "Hkv": HKV, "D": D, "B": B, "len": n,
                          "skipped": "does not fit in device memory"})
                    continue
                gen = torch.Generator(device="cuda").manual_seed(H + B + n)
                q = torch.randn(B, H, D, device="cuda", generator=gen).to(torch.bfloat16)
                lens = torch.full((B,), n, device="cuda", dtype=torch.int32)
                bufs = []
                for _ in range(R):
                    # one sequence of random rows, repeated over the batch: the values do not matter to the clock
                    kv = [torch.randn(n, HKV, D, device="cuda", generator=gen).to(torch.bfloat16) for _ in range(2)]
                    qs = [quantize_rows_e4m3(x.view(-1, D)) for x in kv]
                    bf = [x.unsqueeze(0).repeat(B, 1, 1, 1) for x in kv]
                    codes = [c.view(torch.uint8).view(1, n, HKV, D).repeat(B, 1, 1, 1).view(torch.float8_e4m3fn)
                             for c, _ in qs]
                    scales = [s.view(1, n, HKV).transpose(1, 2).repeat(B, 1, 1).contiguous() for _, s in qs]
                    bufs.append((bf, codes, scales))
                for chunk in a.chunks:
                    variants = {
                        "bf16": lambda i: decode_attention(q, bufs[i][0][0], bufs[i][0][1], lens, chunk=chunk),
                        "bf16_mfma": lambda i: decode_attention(q, bufs[i][0][0], bufs[i][0][1], lens, chunk=chunk,
                                                                kernel="mfma"),
                        "fp8": lambda i: decode_attention(q, bufs[i][1][0], bufs[i][1][1], lens, chunk=chunk,
                                                          k_scale=bufs[i][2][0], v_scale=bufs[i][2][1]),
                    }
                    graphs = {k: _graph_of(fn, R) for k, fn in variants.items()}
                    one = {k: _time_graph(g, 1) for k, (g, _) in graphs.items()}
                    iters = max(1, min(a.iters, int(a.window_ms / max(one.values()))))
                    us = {k: [] for k in variants}
                    for _ in range(a.runs):
                        for k, (g, _) in graphs.items():
                            us[k].append(1e3 * _time_graph(g, iters) / (iters * R))
                    nbytes = {"bf16": 2 * row_bytes, "bf16_mfma": 2 * row_bytes,
                              "fp8": row_bytes + 2 * B * HKV * n * 4}
                    ref = graphs["bf16"][1][0].float()
                    med = {k: statistics.median(v) for k, v in us.items()}
                    emit({"bench": "decode_attn", "H": H, "Hkv": HKV, "D": D, "B": B, "len": n, "chunk": chunk,
                          "cache_buffers": R, "iters": iters, "runs": a.runs,
                          "us": {k: _summary(v) for k, v in us.items()},
                          "cache_GBps": {k: {s: round(nbytes[k] / (1e3 * t), 1) for s, t in
                                             (("median", med[k]), ("at_min_us", min(v)), ("at_max_us", max(v)))}
                                         for k, v in us.items()},
                          "cache_bytes": nbytes, "fp8_speedup": round(med["bf16"] / med["fp8"], 3),
                          "mfma_speedup": round(med["bf16"] / med["bf16_mfma"], 3),
                          "max_abs_diff_mfma_vs_bf16": round(float((graphs["bf16_mfma"][1][0].float() - ref)
                                                                   .abs().max()), 5),
                          "max_abs_diff_fp8_vs_bf16": round(float((graphs["fp8"][1][0].float() - ref).abs().max()), 5),
                          "ref_abs_max": round(float(ref.abs().max()), 4),
                          "note": "device events around graph replays; every launch of a replay reads another cache"})
                    del graphs
                del bufs
                torch.cuda.empty_cache()


def part_shared_kernel(a, emit):
    H, HKV, D, Bp, S = 32, 8, 128, 8, 512
    free = torch.cuda.mem_get_info()[0]
    for n in (1, 4, 8, 16):
        for P in (1024, 8192):
            B = Bp * n
            shared_bytes = 2 * (Bp * P + B * S) * HKV * D * 2     # K and V, prefix + suffix
            rep_bytes = 2 * B * (P + S) * HKV * D * 2
            R = max(2, -(-int(a.min_gb * 2 ** 30) // shared_bytes))
            row = {"bench": "decode_attn_shared", "H": H, "Hkv": HKV, "D": D, "Bp": Bp, "n": n, "prefix": P,
                   "suffix": S}
            if R * (shared_bytes + rep_bytes) > 0.8 * free:
                emit(dict(row, skipped="does not fit in device memory"))
                continue
            gen = torch.Generator(device="cuda").manual_seed(n + P)
            q = torch.randn(B, H, D, device="cuda", generator=gen).to(torch.bfloat16)
            pl = torch.full((Bp,), P, device="cuda", dtype=torch.int32)
            sl = torch.full((B,), S, device="cuda", dtype=torch.int32)
            tl = torch.full((B,), P + S, device="cuda", dtype=torch.int32)
            bufs = []
            for _ in range(R):
                pre = [torch.randn(Bp, P, HKV, D, device="cuda", generator=gen).to(torch.bfloat16) for _ in range(2)]
                suf = [torch.randn(B, S, HKV, D, device="cuda", generator=gen).to(torch.bfloat16) for _ in range(2)]
                full = [torch.cat([x.repeat_interleave(n, 0), y], 1) for x, y in zip(pre, suf)]
                bufs.append((pre, suf, full))
            for chunk in a.chunks:
                variants = {
                    "repeated_mfma": lambda i: decode_attention(q, bufs[i][2][0], bufs[i][2][1], tl, chunk=chunk,
                                                                kernel="mfma"),
                    "shared": lambda i: decode_attention_shared(q, bufs[i][0][0], bufs[i][0][1], pl, bufs[i][1][0],
                                                                bufs[i][1][1], sl, n, chunk=chunk),
                }
                graphs = {k: _graph_of(fn, R) for k, fn in variants.items()}
                one = {k: _time_graph(g, 1) for k, (g, _) in graphs.items()}
                iters = max(1, min(a.iters, int(a.window_ms / max(one.values()))))
                us = {k: [] for k in variants}
                for _ in range(a.runs):
                    for k, (g, _) in graphs.items():
                        us[k].append(1e3 * _time_graph(g, iters) / (iters * R))
                med = {k: statistics.median(v) for k, v in us.items()}
                nbytes = {"repeated_mfma": rep_bytes, "shared": shared_bytes}
                ref = graphs["repeated_mfma"][1][0].float()
                emit(dict(row, chunk=chunk, cache_buffers=R, iters=iters, runs=a.runs,
                          us={k: _summary(v) for k, v in us.items()},
                          cache_GBps={k: round(nbytes[k] / (1e3 * med[k]), 1) for k in us}, cache_bytes=nbytes,
                          byte_ratio=round(rep_bytes / shared_bytes, 3),
                          shared_speedup=round(med["repeated_mfma"] / med["shared"], 3),
                          max_abs_diff_shared_vs_repeated=round(float((graphs["shared"][1][0].float() - ref)
                                                                      .abs().max()), 5),
                          ref_abs_max=round(float(ref.abs().max()), 4),
                          note="device events around graph replays; every launch of a replay reads other caches"))
                del graphs
            del bufs
            torch.cuda.empty_cache()


def part_shared_rollout(a, emit, m):
    cfg = m.cfg
    Bp, n, P, T = a.batch, a.samples, a.prompt, a.new
    p = torch.randint(0, cfg.vocab_size, (Bp, P), device="cuda")
    full = torch.full((Bp,), P, device="cuda")
    kw = dict(temperature=1.0, top_k=50, top_p=0.95, fused_sampling=True, seed=1)
    engines = {k: HybridEngine(m, Bp * n, P + T, use_graph=True, decode_kernel="mfma")
               for k in ("repeated_mfma", "shared")}
    calls = {"repeated_mfma": lambda e, t: e.generate_ragged(p.repeat_interleave(n, 0), full.repeat_interleave(n), t,
                                                             **kw),
             "shared": lambda e, t: e.generate_ragged(p, full, t, samples_per_prompt=n, **kw)}
    for k, e in engines.items():
        calls[k](e, 8)  # warm-up
    total, short = {k: [] for k in engines}, {k: [] for k in engines}
    for _ in range(a.runs):
        for k, e in engines.items():
            short[k].append(_clock(lambda: calls[k](e, 8))[0])
            total[k].append(_clock(lambda: calls[k](e, T))[0])
    # the caches of the last (T-token) call: prefix + suffix for the shared form
    gib = {k: round((e.cache.nbytes + (e.prefix.nbytes if k == "shared" else 0)) / 2 ** 30, 3)
           for k, e in engines.items()}
    emit({"bench": "shared_prefix_rollout_ms_per_token", "model": a.model, "prompts": Bp, "samples_per_prompt": n,
          "prompt": P, "new": T, "top_k": 50, "top_p": 0.95, "graph": True, "fused_sampling": True,
          "fused_kv_append": False, "decode_kernel": "mfma", "runs": a.runs,
          "ms_per_token_whole_call": {k: _summary([t / T for t in v]) for k, v in total.items()},
          "ms_per_token_decode_only": {k: _summary([(t - s) / (T - 8) for t, s in zip(total[k], short[k])])
                                       for k in engines},
          "kv_cache_GiB": gib,
          "note": "host clock around generate_ragged (prefill and capture included) / new tokens; decode_only = "
                  "(t(new) - t(8)) / (new - 8); the suffix cache of the short call is sized for 8 tokens; "
                  "alternating runs"})


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
    engines = {k: HybridEngine(m, B, P + T, use_graph=True, fused_kv_append=True, kv_cache=v, decode_kernel=dk)
               for k, v, dk in (("unset", None, None), ("fp8", "fp8", None), ("bf16_mfma", None, "mfma"))}
    for e in engines.values():
        e.generate_ragged(p, full, 8, **kw)  # warm-up
    total, short = {k: [] for k in engines}, {k: [] for k in engines}
    for _ in range(a.runs):
        for k, e in engines.items():
            short[k].append(_clock(lambda: e.generate_ragged(p, full, 8, **kw))[0])
            total[k].append(_clock(lambda: e.generate_ragged(p, full, T, **kw))[0])
    emit({"bench": "rollout_ms_per_token", "model": a.model, "batch": B, "prompt": P, "new": T, "top_k": 50,
          "top_p": 0.95, "graph": True, "fused_sampling": True, "fused_kv_append": True, "runs": a.runs,
          "ms_per_token_whole_call": {k: _summary([t / T for t in v]) for k, v in total.items()},
          "ms_per_token_decode_only": {k: _summary([(t - s) / (T - 8) for t, s in zip(total[k], short[k])])
                                       for k in engines},
          "kv_cache_GiB": {k: round(e.cache.nbytes / 2 ** 30, 3) for k, e in engines.items()},
          "note": "host clock around generate_ragged (prefill and capture included) / new tokens; decode_only = "
                  "(t(new) - t(8)) / (new - 8), both with the same prompt; alternating runs"})


@torch.no_grad()
def part_distance(a, emit, m, name):
    cfg = m.cfg
    B, P, T = a.batch, min(128, cfg.max_position_embeddings // 4), min(128, cfg.max_position_embeddings // 4)
    p = torch.randint(0, cfg.vocab_size, (B, P), device="cuda")
    eng = HybridEngine(m, B, P + T, use_graph=False, fused_kv_append=True, kv_cache="fp8")
    seq = eng.generate(p, T, temperature=1.0, top_k=50, top_p=0.95, fused_sampling=True, seed=3)
    resp = seq[:, P:]
    # bf16 policy: the full forward that make_experience scores with
    lp_bf16 = torch.log_softmax(m(seq[:, :-1])[:, P - 1:].float(), -1).gather(-1, resp[..., None])[..., 0]
    d = {}
    for k, e in (("fp8_cache", eng), ("bf16_cache", HybridEngine(m, B, P + T, use_graph=False,
                                                               fused_kv_append=True))):
        # the same tokens teacher-forced through the decode path
        e._ensure_cache(B, p.device, torch.bfloat16)
        logits = [e._forward(p, prefill=True)]
        for t in range(T - 1):
            logits.append(e._forward(resp[:, t:t + 1], prefill=False).clone())
        lp = torch.log_softmax(torch.stack(logits, 1).float(), -1).gather(-1, resp[..., None])[..., 0]
        # the first response token comes from the bf16 prefill in both: leave it out
        x = (lp_bf16 - lp).abs()[:, 1:]
        d[k] = {"mean": round(float(x.mean()), 5), "max": round(float(x.max()), 5)}
    emit({"bench": "fp8_kv_cache_policy_distance", "model": name, "weights": "random init", "batch": B,
          "prompt": P, "response_tokens": int(x.numel()), "abs_logp_diff_decode_vs_bf16_forward": d,
          "mean_logp_bf16": round(float(lp_bf16.mean()), 4),
          "note": "sampled with top_k 50 / top_p 0.95 from the fp8-cache engine; log-probs over the full vocabulary"})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/r9/rl_decode_attn_ab.jsonl")
    ap.add_argument("--part", default="all", help="all (kernel, rollout, distance), or a comma list of them and "
                                                  "shared, shared_kernel, shared_rollout")
    ap.add_argument("--samples", type=int, default=8, help="shared: samples per prompt of the rollout row")
    ap.add_argument("--model", default="llama3-8b")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--prompt", type=int, default=4096)
    ap.add_argument("--new", type=int, default=128)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--iters", type=int, default=40, help="most graph replays per timed window")
    ap.add_argument("--window-ms", type=float, default=30.0, help="aimed length of a timed window")
    ap.add_argument("--min-gb", type=float, default=1.0, help="e4m3 cache bytes a replay walks through")
    ap.add_argument("--chunks", type=lambda s: [int(x) for x in s.split(",")], default=[256, 1024])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_rl_decode_attn.py measures on a GPU; none found")
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    f = open(a.out, "w")

    def emit(r):
        line = json.dumps(r)
        print(line, flush=True)
        f.write(line + "\n")
        f.flush()

    parts = {"kernel", "rollout", "distance"} if a.part == "all" else set(a.part.split(","))
    if "shared" in parts:
        parts = parts - {"shared"} | {"shared_kernel", "shared_rollout"}
    if parts - {"kernel", "rollout", "distance", "shared_kernel", "shared_rollout"}:
        sys.exit(f"unknown --part {a.part}")
    if "shared_kernel" in parts:
        part_shared_kernel(a, emit)
    if "kernel" in parts:
        part_kernel(a, emit)
    if "distance" in parts:
        part_distance(a, emit, _model("llama-tiny"), "llama-tiny")
    if "shared_rollout" in parts:
        part_shared_rollout(a, emit, _model(a.model))
    if "rollout" in parts or ("distance" in parts and a.model != "llama-tiny"):
        m = _model(a.model)
        if "rollout" in parts:
            part_rollout(a, emit, m)
        if "distance" in parts and a.model != "llama-tiny":
            part_distance(a, emit, m, a.model)
    f.close()


if __name__ == "__main__":
    main()
