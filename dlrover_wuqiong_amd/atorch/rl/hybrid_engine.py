"""Hybrid engine: the PPO actor generates with a KV cache from the same
weights it trains, switching from the (possibly FSDP-sharded) training
layout to an inference layout and back.

MI355X-first design (vs the reference's DeepSpeed-container swap +
optional vLLM backend):
  * ``gathered_params``: FSDP2 units are unsharded once for the whole
    rollout (one all-gather per unit over RCCL, not one per decoded token)
    and resharded before training resumes; 288 GB of HBM holds an 8B actor's
    full bf16 weights next to its shards, optimizer state and the cache;
  * a static KV cache [L, B, Smax, Hkv, D] in HBM; prefill runs the MFMA flash
    attention over the prompt and writes K/V into the cache; each decode
    step runs the split-KV decode kernel (``ops.attention.decode_attention``,
    ``csrc/kernels/attn_decode.hip``) whose lengths live on the device;
  * the decode step (embedding -> L x {RMSNorm, QKV GEMM, RoPE at the device
    positions, cache scatter, decode attention, O GEMM, RMSNorm, MLP} -> LM
    head, lengths += 1) is captured ONCE in a HIP graph and replayed per
    token, so a token costs one graph launch instead of ~15 kernel launches
    per layer.  Sampling stays outside the graph unless ``fused_sampling``
    is on: then the captured step is "draw from the previous step's logits
    (``ops.sampling``), then forward" and the host only replays.

Works with ``models.llama.Llama`` (dense FFN for graph capture; MoE runs
eagerly), including tensor-parallel actors (each rank caches its own KV
heads, the TP layers do their own RCCL collectives, the vocab-parallel LM
head's logits are all-gathered before sampling; decoded eagerly: no graph
around collectives) and sequence-parallel actors (weights are replicated
over the SP group, so generation runs with SP switched off and every SP rank
produces the same rollout).  Parity: ATorch ``atorch/rl/ds_hybrid_engine/hybrid_engine.py``
(generate with gathered ZeRO-3 params, inference containers, KV cache) and
``rl/inference_backend/vllm_backend.py``.
"""

import contextlib
from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from ...common.log import logger
from ...ops import skinny_gemm
from ...ops.activation import swiglu
from ...ops.attention import decode_attention, flash_attn_func
from ...ops.rollout import kv_append_rope, rollout_step
from ...ops.rope import apply_rope, rope_table


def find_llama(model: nn.Module):
    """The ``models.llama.Llama`` inside ``model`` (wrappers such as the
    autocast module of ``auto_accelerate`` or FSDP2 keep it as a submodule)."""
    from ...models.llama import Llama

    for m in model.modules():
        if isinstance(m, Llama):
            return m
    return None


@contextlib.contextmanager
def gathered_params(model: nn.Module):
    """Unshard every FSDP2 unit of ``model`` for the duration (no-op for an
    unsharded model)."""
    try:
        from torch.distributed.fsdp import FSDPModule
    except ImportError:  # pragma: no cover
        FSDPModule = ()
    units = [m for m in model.modules() if FSDPModule and isinstance(m, FSDPModule)]
    for u in units:
        u.unshard()
    try:
        yield
    finally:
        for u in units:
            u.reshard()


class KVCache:
    def __init__(self, n_layers: int, batch: int, max_len: int, n_kv: int, head_dim: int, device, dtype):
        self.k = torch.zeros(n_layers, batch, max_len, n_kv, head_dim, device=device, dtype=dtype)
        self.v = torch.zeros_like(self.k)
        self.lens = torch.zeros(batch, device=device, dtype=torch.int32)
        self.max_len = max_len

    @property
    def nbytes(self) -> int:
        return 2 * self.k.numel() * self.k.element_size()


class HybridEngine:
    def __init__(self, actor: nn.Module, max_batch: int, max_len: int, use_graph: bool = True,
                 fused_kv_append: bool = False, rollout_weights: Optional[str] = None):
        """``fused_kv_append`` (bf16 GPU actors): the decode step's QKV split,
        RoPE and K/V cache write are one launch per layer
        (``ops.rollout.kv_append_rope``) instead of the split / rope /
        index_copy_ chain.

        ``rollout_weights`` (dense actors on one rank; docs/rl_fp8_rollouts.md):
        the decode step's five GEMMs (qkv, o, gate|up, down, LM head) run
        ``ops.skinny_gemm.skinny_linear`` -- ``"bf16"`` on the live weights,
        ``"fp8"`` on e4m3 copies of the four layer weights that are refilled
        at the start of every ``generate`` / ``generate_ragged`` (the LM head
        stays bf16).  Prefill keeps the module's own GEMMs.  With ``"fp8"``
        the rollout is sampled from a slightly different policy than the bf16
        one that scores it afterwards."""
        self.actor = actor
        self.llama = find_llama(actor)
        if self.llama is None:
            raise TypeError("HybridEngine drives models.llama.Llama actors")
        from ...models.llama import _ws

        self.tp_group = getattr(self.llama, "tp_group", None)
        self.tp = _ws(self.tp_group)
        cfg = self.llama.cfg
        self.cfg = cfg
        self.max_batch, self.max_len = max_batch, max_len
        self.use_graph = use_graph and cfg.num_experts == 0 and self.tp == 1
        self.fused_kv_append = fused_kv_append
        if rollout_weights not in (None, "bf16", "fp8"):
            raise ValueError(f"rollout_weights must be None, 'bf16' or 'fp8', got {rollout_weights!r}")
        if rollout_weights is not None and (self.tp > 1 or cfg.num_experts > 0):
            raise ValueError("rollout_weights covers dense single-rank actors: tensor-parallel and MoE actors "
                             "are not covered")
        self.rollout_weights = rollout_weights
        self._wq = {}   # "fp8": layer linear -> (codes [N, K] e4m3, scale fp32 [N]), allocated once
        self._gemm_ws = None   # split-K scratch of the streaming GEMMs, sized by the eager decode step
        if rollout_weights is not None:
            for name, lin in self._decode_linears():
                self._check_streamable(name, lin)
        self.cache: Optional[KVCache] = None
        self._graph = None
        self._graph_key = None
        self._tok = None
        self._logits = None
        self.token_steps = 0

    # ------------------------------------------------------------ forward
    def _ensure_cache(self, B: int, device, dtype):
        c = self.cache
        if c is None or c.k.shape[1] != B or c.k.device != device or c.k.dtype != dtype:
            cfg = self.cfg
            # this rank's KV heads (all of them without tensor parallelism)
            self.cache = KVCache(cfg.num_hidden_layers, B, self.max_len, cfg.num_key_value_heads // self.tp,
                                 cfg.head_dim, device, dtype)
            self._graph = None
            logger.info(f"hybrid engine: KV cache {self.cache.nbytes / 2**30:.2f} GiB "
                        f"({B} x {self.max_len} tokens)")
        return self.cache

    def _decode_linears(self):
        """(name, module) of the decode step's GEMMs that ``rollout_weights``
        reroutes: four per layer and the untied head."""
        for li, layer in enumerate(self.llama.layers):
            for name, lin in (("self_attn.qkv_proj", layer.self_attn.qkv_proj),
                              ("self_attn.o_proj", layer.self_attn.o_proj),
                              ("mlp.gate_up_proj", getattr(layer.mlp, "gate_up_proj", None)),
                              ("mlp.down_proj", getattr(layer.mlp, "down_proj", None))):
                yield f"layers.{li}.{name}", lin
        if self.llama.lm_head is not None:
            yield "lm_head", self.llama.lm_head

    @staticmethod
    def _check_streamable(name, lin):
        """``y = x W^T`` from ``lin.weight`` alone is what the module
        computes: a bias-free ``nn.Linear`` with its own forward.  A wrapper
        that adds to it (an unmerged LoRA adapter, a bias) must not be dropped
        from the decode steps only."""
        if not (isinstance(lin, nn.Linear) and type(lin).forward is nn.Linear.forward and lin.bias is None):
            raise ValueError(f"rollout_weights needs plain bias-free nn.Linear layers; {name} is "
                             f"{type(lin).__name__} (merge LoRA adapters first, or leave rollout_weights unset)")

    def _refresh_rollout_weights(self):
        """``"fp8"``: requantise the layer weights into the engine's buffers
        (training changed them since the last rollout).  Runs inside
        ``gathered_params``, where every weight is whole."""
        if self.rollout_weights != "fp8":
            return
        for name, lin in self._decode_linears():
            if lin is self.llama.lm_head:
                continue   # the head stays bf16
            self._check_streamable(name, lin)
            w = lin.weight.detach()
            buf = self._wq.get(lin)
            if buf is None or buf[0].shape != w.shape or buf[0].device != w.device:
                buf = self._wq[lin] = (torch.empty(w.shape, device=w.device, dtype=torch.float8_e4m3fn),
                                       torch.empty(w.shape[0], device=w.device, dtype=torch.float32))
            skinny_gemm.quantize_rows_e4m3(w, out=buf)

    def _stream(self, x, w, scale=None):
        """``skinny_linear`` on the engine's own split-K scratch.  It grows in
        the eager decode step that precedes a capture (the captured step has
        the same shapes), so nothing is allocated while a graph records; the
        engine's streams are ordered, so one buffer serves them all."""
        if x.is_cuda:
            need = skinny_gemm.workspace_floats(x.numel() // x.shape[-1], w.shape[0], w.shape[1],
                                                w.dtype == torch.float8_e4m3fn)
            if need and (self._gemm_ws is None or self._gemm_ws.numel() < need
                         or self._gemm_ws.device != x.device):
                self._gemm_ws = torch.empty(need, device=x.device, dtype=torch.float32)
        return skinny_gemm.skinny_linear(x, w, scale, workspace=self._gemm_ws)

    def _lin(self, lin, x, prefill: bool):
        """A bias-free linear of the actor: the module's own GEMM, or in a
        decode step with ``rollout_weights`` the weight-streaming one."""
        if prefill or self.rollout_weights is None:
            return lin(x)
        self._check_streamable(type(lin).__name__, lin)   # wrapped after the engine was built
        if self.rollout_weights == "fp8":
            q = self._wq.get(lin)
            if q is None:
                raise RuntimeError("rollout_weights='fp8': no e4m3 copy of this layer yet; generate / "
                                   "generate_ragged make them (_refresh_rollout_weights)")
            return self._stream(x, q[0], q[1])
        return self._stream(x, lin.weight)

    def _mlp(self, mlp, x, prefill: bool):
        if prefill or self.rollout_weights is None:
            return mlp(x)
        return self._lin(mlp.down_proj, swiglu(self._lin(mlp.gate_up_proj, x, prefill)), prefill)

    def _layer(self, li: int, layer, x, r, cos, sin, pos_ids, prefill: bool):
        attn = layer.self_attn
        if r is None:
            a, h = layer.input_layernorm(x), x
        else:
            a, h = layer.input_layernorm.add_forward(x, r)
        B, S, _ = a.shape
        qkv = self._lin(attn.qkv_proj, a, prefill).view(B, S, attn.nh + 2 * attn.nkv, attn.hd)
        c = self.cache
        if self.fused_kv_append and not prefill and qkv.is_cuda and qkv.dtype == torch.bfloat16:
            q = kv_append_rope(qkv, attn.nh, attn.nkv, cos, sin, c.k[li], c.v[li], c.lens)
            y = decode_attention(q.view(B, attn.nh, attn.hd), c.k[li], c.v[li], c.lens + 1)
            b, h = layer.post_attention_layernorm.add_forward(
                h, self._lin(attn.o_proj, y.view(B, 1, attn.nh * attn.hd), prefill))
            return h, self._mlp(layer.mlp, b, prefill)
        q, k, v = qkv.split([attn.nh, attn.nkv, attn.nkv], dim=2)
        q = apply_rope(q.contiguous(), cos, sin, pos_ids)
        k = apply_rope(k.contiguous(), cos, sin, pos_ids)
        if prefill:
            c.k[li, :B, :S] = k
            c.v[li, :B, :S] = v
            y = flash_attn_func(q, k, v.contiguous(), causal=True).reshape(B, S, attn.nh * attn.hd)
        else:
            # scatter this token's K/V at each sequence's length (device index)
            idx = (torch.arange(B, device=a.device, dtype=torch.int64) * self.max_len + c.lens.to(torch.int64))
            c.k[li].view(B * self.max_len, attn.nkv, attn.hd).index_copy_(0, idx, k.view(B, attn.nkv, attn.hd))
            c.v[li].view(B * self.max_len, attn.nkv, attn.hd).index_copy_(0, idx, v.reshape(B, attn.nkv, attn.hd))
            y = decode_attention(q.view(B, attn.nh, attn.hd), c.k[li], c.v[li], c.lens + 1)
            y = y.view(B, 1, attn.nh * attn.hd)
        b, h = layer.post_attention_layernorm.add_forward(h, self._lin(attn.o_proj, y, prefill))
        return h, self._mlp(layer.mlp, b, prefill)

    def _forward(self, ids, prefill: bool, last=None):
        """``last`` (prefill of ragged prompts): int64 [B], the column of each
        row's last real token; its logits are returned and the cache lengths
        become ``last + 1``."""
        m, cfg = self.llama, self.cfg
        B, S = ids.shape
        x = m.embed_tokens(ids)
        cos, sin = rope_table(self.max_len, cfg.head_dim, cfg.rope_theta, x.device)
        pos_ids = None if prefill else self.cache.lens.view(B, 1)
        r = None
        for li, layer in enumerate(m.layers):
            x, r = self._layer(li, layer, x, r, cos, sin, pos_ids, prefill)
        x = m.norm.add_forward(x, r)[0]
        x = x[:, -1] if last is None else x[torch.arange(B, device=x.device), last]
        if prefill or self.rollout_weights is None:
            logits = F.linear(x, m.embed_tokens.weight) if m.lm_head is None else m.lm_head(x)
        else:
            # the head stays bf16 in both modes: these logits are sampled from
            if m.lm_head is not None:
                self._check_streamable("lm_head", m.lm_head)
            logits = self._stream(x, (m.embed_tokens if m.lm_head is None else m.lm_head).weight)
        if self.tp > 1:
            # vocab-parallel head: every rank samples from the full vocabulary
            import torch.distributed as dist

            parts = [torch.empty_like(logits) for _ in range(self.tp)]
            dist.all_gather(parts, logits.contiguous(), group=self.tp_group)
            logits = torch.cat(parts, -1)[:, :cfg.vocab_size]
        if last is not None:
            self.cache.lens.copy_(last + 1)
        elif prefill:
            self.cache.lens.fill_(S)
        else:
            self.cache.lens.add_(1)
        return logits

    def prefill(self, prompts: torch.Tensor) -> torch.Tensor:
        B, P = prompts.shape
        if B > self.max_batch or P >= self.max_len:
            raise ValueError(f"prompts [{B}, {P}] exceed the engine ({self.max_batch}, {self.max_len})")
        dtype = self.llama.embed_tokens.weight.dtype
        self._ensure_cache(B, prompts.device, dtype)
        return self._forward(prompts, prefill=True)

    def decode(self, tok: torch.Tensor) -> torch.Tensor:
        """tok [B, 1] -> next-token logits [B, V] (graph replay when captured)."""
        if self._graph is not None:
            self._tok.copy_(tok)
            self._graph.replay()
            return self._logits
        return self._forward(tok, prefill=False)

    def _capture(self, tok: torch.Tensor):
        """Capture one decode step (the current state is not advanced:
        capture records kernels without running them)."""
        self._tok = tok.clone()
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            with torch.cuda.graph(g, stream=s):
                self._logits = self._forward(self._tok, prefill=False)
        torch.cuda.current_stream().wait_stream(s)
        self._graph = g

    def _capture_sampled(self, logits: torch.Tensor, sampler):
        """Capture "sample from the previous step's logits, then forward":
        ``_logits`` is the step's input and output, ``_tok`` the token it
        drew.  Nothing runs during capture."""
        self._logits = logits.clone()
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            with torch.cuda.graph(g, stream=s):
                self._tok = sampler(self._logits)
                self._logits.copy_(self._forward(self._tok, prefill=False))
        torch.cuda.current_stream().wait_stream(s)
        self._graph = g

    def _generate_fused(self, prompts, max_new_tokens, sampler):
        """The rollout loop with the fused sampler: with a graph the host only
        replays and clones the token buffer."""
        out = [prompts]
        logits = self.prefill(prompts)
        for t in range(max_new_tokens):
            if self._graph is not None and t < max_new_tokens - 1:
                self._graph.replay()
                out.append(self._tok.clone())
                continue
            # the first token, the last one (no forward after it: the cache
            # ends at prompt + generated - 1), and every token without a graph
            nxt = sampler(self._logits if self._graph is not None else logits)
            if self.tp > 1:
                import torch.distributed as dist

                dist.broadcast(nxt, dist.get_global_rank(self.tp_group, 0), group=self.tp_group)
            out.append(nxt)
            if t == max_new_tokens - 1:
                break
            logits = self._forward(nxt, prefill=False)
            if t == 0 and self.use_graph:
                # that was the eager step that allocates every workspace
                self._capture_sampled(logits, sampler)
        return out

    # ----------------------------------------------------------- generate
    @torch.no_grad()
    def generate(self, prompts: torch.Tensor, max_new_tokens: int, temperature: float = 1.0, top_k: int = 0,
                 generator: Optional[torch.Generator] = None, top_p: float = 1.0, fused_sampling: bool = False,
                 seed: Optional[int] = None) -> torch.Tensor:
        """``fused_sampling`` (GPU, ``temperature > 0``): every token is drawn
        by ``ops.sampling.sample_tokens`` from ``seed`` (default 0) and a
        device-side call counter that starts at 0, so a call is reproducible;
        with ``use_graph`` the draw is part of the captured decode step."""
        B, P = prompts.shape
        if P + max_new_tokens > self.max_len:
            raise ValueError(f"{P} + {max_new_tokens} tokens exceed the cache ({self.max_len})")
        was_training = self.actor.training
        self.actor.eval()
        out = [prompts]
        sp_saved = getattr(self.llama, "sp_group", None)
        if sp_saved is not None:
            self.llama.set_sp(1, 0, None)  # replicated weights: decode without the SP all-to-alls
        try:
            with gathered_params(self.actor):
                self._graph = None
                self._refresh_rollout_weights()
                if fused_sampling and temperature > 0 and prompts.is_cuda:
                    from ...ops.sampling import sample_tokens

                    offset = torch.zeros(1, device=prompts.device, dtype=torch.int64)
                    out = self._generate_fused(prompts, max_new_tokens, lambda lg: sample_tokens(
                        lg, temperature, top_k, top_p, seed=seed or 0, offset=offset))
                    max_new_tokens = 0
                else:
                    logits = self.prefill(prompts)
                for t in range(max_new_tokens):
                    nxt = _sample(logits.float(), temperature, top_k, generator, top_p)
                    if self.tp > 1:
                        # one sample per TP group: the ranks decode the same sequence
                        import torch.distributed as dist

                        dist.broadcast(nxt, dist.get_global_rank(self.tp_group, 0), group=self.tp_group)
                    out.append(nxt)
                    if t == max_new_tokens - 1:
                        break
                    if t == 0 and self.use_graph and prompts.is_cuda:
                        # one eager step (allocates every workspace), then
                        # record the step; capture does not advance the state
                        logits = self._forward(nxt, prefill=False)
                        self._capture(nxt)
                        continue
                    logits = self.decode(nxt)
                # captured against this call's weights / cache: never replayed later
                self._graph = None
        finally:
            if sp_saved is not None:
                import torch.distributed as dist

                self.llama.set_sp(dist.get_world_size(sp_saved), dist.get_rank(sp_saved), sp_saved)
            self.actor.train(was_training)
        return torch.cat(out, 1)

    # ---------------------------------------------------- ragged generate
    def _capture_ragged(self, step, nxt):
        """Capture one ragged token step; ``step(nxt)`` records "[sample,]
        rollout_step, forward" on the engine's persistent buffers."""
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            with torch.cuda.graph(g, stream=s):
                self._logits.copy_(step(nxt))
        torch.cuda.current_stream().wait_stream(s)
        self._graph = g

    @torch.no_grad()
    def generate_ragged(self, prompts: torch.Tensor, prompt_lens: torch.Tensor, max_new_tokens: int,
                        temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0,
                        generator: Optional[torch.Generator] = None, fused_sampling: bool = False,
                        seed: Optional[int] = None, eos_token_id: Optional[int] = None, pad_token_id: int = 0,
                        eos_check_interval: int = 8):
        """Rollout of prompts of different lengths that may stop at an EOS.

        ``prompts`` [B, Pmax] is left-aligned: row ``b`` holds its
        ``prompt_lens[b]`` real tokens first (``1 <= p_b <= Pmax``), anything
        after them.  Returns ``(seq [B, Pmax + max_new_tokens], prompt_lens,
        response_lens)`` with ``seq[b] = prompt_b | response_b | pad...``;
        ``response_lens`` counts the EOS token.

        Causal attention never looks right of a token and every row's
        positions start at 0, so no mask is needed: the prefill is one dense
        pass over [B, Pmax] whose logits are read at column ``p_b - 1``, the
        cache lengths start at ``prompt_lens`` (the pads' K/V lie beyond them
        and are overwritten as the row grows), and each token is written at
        its row's own column by ``ops.rollout.rollout_step``.  A finished row
        keeps decoding ``pad_token_id``; the host reads the count of
        unfinished rows every ``eos_check_interval`` tokens and stops at 0.
        With ``use_graph`` the captured step is "sample, rollout_step,
        forward" (greedy or ``fused_sampling``; a torch-sampled token is drawn
        by the host in front of the replay)."""
        B, Pmax = prompts.shape
        L = Pmax + max_new_tokens
        if L > self.max_len:
            raise ValueError(f"{Pmax} + {max_new_tokens} tokens exceed the cache ({self.max_len})")
        if B > self.max_batch:
            raise ValueError(f"{B} prompts exceed the engine's batch ({self.max_batch})")
        dev = prompts.device
        prompt_lens = torch.as_tensor(prompt_lens, device=dev).to(torch.int64).view(B)
        if int(prompt_lens.min()) < 1 or int(prompt_lens.max()) > Pmax:
            raise ValueError(f"prompt_lens must lie in [1, {Pmax}]")
        eos_check_interval = max(1, int(eos_check_interval))
        was_training = self.actor.training
        self.actor.eval()
        sp_saved = getattr(self.llama, "sp_group", None)
        if sp_saved is not None:
            self.llama.set_sp(1, 0, None)  # replicated weights: decode without the SP all-to-alls
        # the cells right of a prompt are never attended to: make them pad
        real = torch.arange(Pmax, device=dev).view(1, Pmax) < prompt_lens.view(B, 1)
        seq = torch.full((B, L), int(pad_token_id), device=dev, dtype=torch.int64)
        seq[:, :Pmax] = torch.where(real, prompts.to(torch.int64), seq[:, :Pmax])
        finished = torch.zeros(B, device=dev, dtype=torch.int32)
        resp_len = torch.zeros(B, device=dev, dtype=torch.int32)
        n_active = torch.full((1,), B, device=dev, dtype=torch.int32)
        self._tok = torch.zeros(B, 1, device=dev, dtype=torch.int64)
        fused = bool(fused_sampling and temperature > 0 and prompts.is_cuda)
        if fused:
            from ...ops.sampling import sample_tokens

            offset = torch.zeros(1, device=dev, dtype=torch.int64)

            def sampler(lg):
                return sample_tokens(lg, temperature, top_k, top_p, seed=seed or 0, offset=offset)
        else:
            def sampler(lg):
                return _sample(lg.float(), temperature, top_k, generator, top_p)
        # a graph records the draw when it needs no host state
        in_graph = fused or temperature <= 0

        def step(nxt):
            """[sample,] place the token / latch EOS, forward what the rows read next."""
            if nxt is None:
                nxt = sampler(self._logits)
            rollout_step(nxt, self.cache.lens, finished, resp_len, seq, self._tok, n_active, eos_token_id,
                         pad_token_id)
            return self._forward(self._tok, prefill=False)

        try:
            with gathered_params(self.actor):
                self._graph = None
                self._refresh_rollout_weights()
                dtype = self.llama.embed_tokens.weight.dtype
                self._ensure_cache(B, dev, dtype)
                logits = self._forward(seq[:, :Pmax], prefill=True, last=prompt_lens - 1)
                nxt_buf = None
                for t in range(max_new_tokens):
                    if self._graph is not None and t < max_new_tokens - 1:
                        if not in_graph:
                            nxt_buf.copy_(sampler(self._logits))
                        self._graph.replay()
                    else:
                        nxt = sampler(self._logits if self._graph is not None else logits)
                        if self.tp > 1:
                            # one sample per TP group: the ranks decode the same sequence
                            import torch.distributed as dist

                            dist.broadcast(nxt, dist.get_global_rank(self.tp_group, 0), group=self.tp_group)
                        rollout_step(nxt, self.cache.lens, finished, resp_len, seq, self._tok, n_active,
                                     eos_token_id, pad_token_id)
                        if t == max_new_tokens - 1:
                            self.token_steps = max_new_tokens
                            break  # the last token is not forwarded
                        logits = self._forward(self._tok, prefill=False)
                        if t == 0 and self.use_graph and prompts.is_cuda:
                            # that was the eager step that allocates every workspace
                            self._logits = logits.clone()
                            nxt_buf = None if in_graph else nxt.clone()
                            self._capture_ragged(step, nxt_buf)
                    self.token_steps = t + 1   # token steps this rollout ran (<= max_new_tokens)
                    if eos_token_id is not None and (t + 1) % eos_check_interval == 0 and int(n_active) == 0:
                        break
                # captured against this call's weights / cache: never replayed later
                self._graph = None
        finally:
            if sp_saved is not None:
                import torch.distributed as dist

                self.llama.set_sp(dist.get_world_size(sp_saved), dist.get_rank(sp_saved), sp_saved)
            self.actor.train(was_training)
        return seq, prompt_lens, resp_len.to(torch.int64)


def _sample(logits: torch.Tensor, temperature: float, top_k: int, generator, top_p: float = 1.0) -> torch.Tensor:
    if temperature <= 0:
        return logits.argmax(-1, keepdim=True)
    if top_p < 1.0:
        from ...ops.sampling import sample_tokens

        return sample_tokens(logits, temperature, top_k, top_p, generator=generator)
    logits = logits / temperature
    if top_k:
        kth = logits.topk(top_k, dim=-1).values[:, -1:]
        logits = logits.masked_fill(logits < kth, float("-inf"))
    return torch.multinomial(logits.softmax(-1), 1, generator=generator)
