"""The decode step's bookkeeping for RL rollouts (``csrc/kernels/rollout.hip``).

``kv_append_rope``: split of a packed QKV projection + RoPE on q and k + append
of k and v into a static KV cache at each row's own length, one launch.
``rollout_step``: what follows the sampler in a ragged rollout with an EOS
token, one launch.  Both are forward only (rollouts run under ``no_grad``) and
have a torch implementation for CPU / non-bf16 tensors, which is also the
reference of the GPU tests.
"""

import torch

from . import _hip
from .rope import _table, apply_rope


def _check_cache(qkv, nh, nkv, k_cache, v_cache, lens):
    if qkv.dim() != 4 or qkv.shape[2] != nh + 2 * nkv or nh < 1 or nkv < 1:
        raise _hip.HipKernelError(f"kv_append_rope expects qkv [B, S, {nh} + 2*{nkv}, D], got {tuple(qkv.shape)}")
    B, S, _, D = qkv.shape
    if D % 16:
        raise _hip.HipKernelError(f"kv_append_rope needs head_dim % 16 == 0, got {D}")
    for name, c in (("k_cache", k_cache), ("v_cache", v_cache)):
        if c.dim() != 4 or c.shape[0] != B or c.shape[2:] != (nkv, D):
            raise _hip.HipKernelError(f"{name} must be [{B}, Smax, {nkv}, {D}], got {tuple(c.shape)}")
        if c.dtype != qkv.dtype or c.device != qkv.device:
            raise _hip.HipKernelError(f"{name} is {c.dtype} on {c.device}, qkv {qkv.dtype} on {qkv.device}")
        if c.stride(3) != 1 or c.stride(2) != D:
            raise _hip.HipKernelError(f"{name}: heads x head_dim must be dense, strides {c.stride()}")
    if k_cache.shape != v_cache.shape or k_cache.stride() != v_cache.stride():
        raise _hip.HipKernelError("k_cache and v_cache must share shape and strides")
    if lens is not None:
        if lens.numel() != B or lens.dtype != torch.int32 or lens.device != qkv.device:
            raise _hip.HipKernelError(f"lens must be int32 [{B}] on {qkv.device} "
                                      f"(got {lens.dtype} {tuple(lens.shape)} on {lens.device})")


def _kv_append_rope_ref(qkv, nh, nkv, cos, sin, k_cache, v_cache, lens):
    """The unfused chain: split, two ropes at the rows' positions, cache
    writes.  A token at a position past the cache writes nothing."""
    B, S, _, D = qkv.shape
    Smax = k_cache.shape[1]
    q, k, v = qkv.split([nh, nkv, nkv], dim=2)
    if lens is None:
        q, k = apply_rope(q.contiguous(), cos, sin), apply_rope(k.contiguous(), cos, sin)
        n = min(S, Smax)
        k_cache[:, :n] = k[:, :n]
        v_cache[:, :n] = v[:, :n]
        return q
    pos = lens.to(torch.int64).view(B, 1) + torch.arange(S, device=qkv.device)
    pos_ids = pos.clamp(0, cos.shape[0] - 1)
    q, k = apply_rope(q.contiguous(), cos, sin, pos_ids), apply_rope(k.contiguous(), cos, sin, pos_ids)
    ok = (pos >= 0) & (pos < Smax)
    rows = torch.arange(B, device=qkv.device).view(B, 1).expand(B, S)
    if S == 1:
        # no host read of ``ok`` (graph capture): a row past the cache rewrites
        # what its last slot holds
        slot = pos.clamp(0, Smax - 1)
        keep = ok.view(B, 1, 1, 1)
        k_cache[rows, slot] = torch.where(keep, k, k_cache[rows, slot])
        v_cache[rows, slot] = torch.where(keep, v, v_cache[rows, slot])
    else:
        k_cache[rows[ok], pos[ok]] = k[ok]
        v_cache[rows[ok], pos[ok]] = v[ok]
    return q


def kv_append_rope(qkv, nh: int, nkv: int, cos, sin, k_cache, v_cache, lens=None):
    """qkv ``[B, S, nh + 2 nkv, D]`` (heads ordered q | k | v) -> rotated q
    ``[B, S, nh, D]`` (contiguous); rotated k and plain v are written into
    ``k_cache`` / ``v_cache`` ``[B, Smax, nkv, D]`` (any batch / row strides,
    heads x D dense) in place.

    Token ``(b, s)`` has position ``lens[b] + s`` (``lens`` int32 ``[B]`` on
    the device; ``None``: position ``s``).  The cos / sin row is clamped to the
    table; a token at a position ``>= Smax`` writes no K/V.  Decode is
    ``S = 1``, prefill ``S = P`` without ``lens``.  q and k equal
    ``rope.qkv_split_rope``'s bit for bit."""
    _check_cache(qkv, nh, nkv, k_cache, v_cache, lens)
    if not (_hip.use_hip(qkv) and qkv.dtype == torch.bfloat16):
        return _kv_append_rope_ref(qkv, nh, nkv, cos, sin, k_cache, v_cache, lens)
    qkv = qkv.contiguous()
    B, S, _, D = qkv.shape
    q4 = qkv[:, :, :nh]
    pid = None if lens is None else lens.view(B, 1).expand(B, S)
    cos, sin = _table(cos, q4, pid), _table(sin, q4, pid)
    bs, rs = k_cache.stride(0), k_cache.stride(1)
    if bs % 8 or rs % 8 or k_cache.data_ptr() % 16 or v_cache.data_ptr() % 16:
        raise _hip.HipKernelError(f"kv_append_rope: cache strides ({bs}, {rs}) / base not 16-byte aligned")
    if rs < nkv * D or (B > 1 and bs < rs * k_cache.shape[1]):
        raise _hip.HipKernelError(f"kv_append_rope: overlapping cache strides ({bs}, {rs})")
    q = torch.empty(B, S, nh, D, device=qkv.device, dtype=qkv.dtype)
    _hip.check(_hip.lib().dw_kv_append_rope(_hip.ptr(qkv), _hip.ptr(q), _hip.ptr(k_cache), _hip.ptr(v_cache),
                                            _hip.ptr(cos), _hip.ptr(sin), _hip.ptr(lens), B, S, nh, nkv, D,
                                            k_cache.shape[1], max(bs, rs * k_cache.shape[1]), rs, cos.shape[0],
                                            _hip.stream()), "kv_append_rope")
    return q


def _check_step(sampled, lens, finished, resp_len, seq, tok_out, n_active):
    if seq.dim() != 2 or seq.dtype != torch.int64 or not seq.is_contiguous():
        raise _hip.HipKernelError(f"rollout_step: seq must be contiguous int64 [B, L], got {seq.dtype} "
                                  f"{tuple(seq.shape)}")
    B, dev = seq.shape[0], seq.device
    for name, t, dt, n in (("sampled", sampled, torch.int64, B), ("tok_out", tok_out, torch.int64, B),
                           ("lens", lens, torch.int32, B), ("finished", finished, torch.int32, B),
                           ("resp_len", resp_len, torch.int32, B), ("n_active", n_active, torch.int32, 1)):
        if t.dtype != dt or t.numel() != n or t.device != dev or not t.is_contiguous():
            raise _hip.HipKernelError(f"rollout_step: {name} must be contiguous {dt} with {n} elements on {dev} "
                                      f"(got {t.dtype} {tuple(t.shape)} on {t.device})")


def rollout_step(sampled, lens, finished, resp_len, seq, tok_out, n_active, eos_token_id=None, pad_token_id=0):
    """One token of a ragged rollout, after the sampler.  Per row ``b``:

    * ``tok = pad_token_id if finished[b] else sampled[b]``;
    * ``seq[b, lens[b]] = tok`` when ``lens[b] < L`` (``lens``: the column this
      token lands in = the cache length before it is forwarded);
    * ``resp_len[b] += 1`` for rows not finished before;
    * ``finished[b] |= tok == eos_token_id`` (``None``: no EOS);
    * ``tok_out[b] = tok``, the buffer the next forward reads;

    and ``n_active[0]`` = the number of unfinished rows after the update.
    ``sampled`` / ``tok_out`` int64 with B elements, ``lens`` / ``finished`` /
    ``resp_len`` int32 ``[B]``, ``seq`` int64 ``[B, L]``, ``n_active`` int32
    ``[1]``; everything but ``sampled`` and ``lens`` is updated in place.
    Returns ``tok_out``."""
    _check_step(sampled, lens, finished, resp_len, seq, tok_out, n_active)
    B, L = seq.shape
    eos = -1 if eos_token_id is None else int(eos_token_id)
    if _hip.use_hip(seq):
        _hip.check(_hip.lib().dw_rollout_step(_hip.ptr(sampled), _hip.ptr(lens), _hip.ptr(finished),
                                              _hip.ptr(resp_len), _hip.ptr(seq), _hip.ptr(tok_out),
                                              _hip.ptr(n_active), B, L, eos, int(pad_token_id), _hip.stream()),
                   "rollout_step")
        return tok_out
    fin = finished.bool()
    tok = torch.where(fin, torch.full_like(sampled.view(B), int(pad_token_id)), sampled.view(B))
    col = lens.to(torch.int64)
    ok = (col >= 0) & (col < L)
    rows = torch.arange(B, device=seq.device)
    seq[rows[ok], col[ok]] = tok[ok]
    resp_len += (~fin).to(torch.int32)
    finished.copy_((fin | (tok == eos)).to(torch.int32))
    tok_out.view(B).copy_(tok)
    n_active.copy_((finished == 0).sum().to(torch.int32).view(1))
    return tok_out
