"""Temperature / top-k / top-p token sampling (``csrc/kernels/sample.hip``).

``keep_mask`` is the definition of the kept set that the kernel and the tests
share; ``sample_tokens`` draws one token per row, on the GPU with one fused,
graph-capturable launch when a ``seed`` is given, otherwise with torch ops and
a ``torch.Generator`` (the CPU / gloo path).
"""

import torch

from . import _hip


def keep_mask(logits, temperature, top_k=0, top_p=1.0):
    """bool ``[B, V]``: the tokens sampling may return.  With ``z = x / T`` in
    fp32, in HF order:

    * top-k (``k > 0``): ``z >=`` the k-th largest value; ties at the
      threshold are all kept;
    * top-p (``p < 1``), over what top-k kept: token j is kept iff the kept
      mass strictly above it is below ``p``:
      ``sum_{i kept, z_i > z_j} e^{z_i} < p * sum_{i kept} e^{z_i}``.  Tied
      tokens are kept or dropped together; the most probable one is always
      kept.

    The kept set is ``{z >= tau}`` for one threshold ``tau``."""
    z = logits.float() / temperature
    V = z.shape[-1]
    keep = torch.ones_like(z, dtype=torch.bool)
    if top_k and 0 < top_k < V:
        keep = z >= z.topk(top_k, dim=-1).values[..., -1:]
    if top_p < 1.0:
        zs, _ = z.masked_fill(~keep, float("-inf")).sort(dim=-1, descending=True)
        w = (zs.double() - zs[..., :1].double()).exp()
        above = w.cumsum(-1) - w  # mass before each sorted position
        # a tie group shares the mass above its first member
        pos = torch.arange(V, device=z.device).expand_as(zs)
        first = torch.ones_like(zs, dtype=torch.bool)
        first[..., 1:] = zs[..., 1:] != zs[..., :-1]
        start = torch.where(first, pos, torch.zeros_like(pos)).cummax(-1).values
        above = above.gather(-1, start)
        kept_sorted = (above < top_p * w.sum(-1, keepdim=True)) | (above == 0)
        tau = zs.masked_fill(~kept_sorted, float("inf")).min(-1, keepdim=True).values
        keep = keep & (z >= tau)
    return keep


def _sample_hip(logits, temperature, top_k, top_p, seed, offset):
    if logits.dim() != 2:
        raise ValueError(f"sample_tokens expects [B, V] logits, got {tuple(logits.shape)}")
    B, V = logits.shape
    if logits.dtype not in (torch.bfloat16, torch.float32):
        logits = logits.float()
    if V > 1 and logits.stride(1) != 1:
        logits = logits.contiguous()
    if offset is None:
        offset = torch.zeros(1, device=logits.device, dtype=torch.int64)
    if offset.dtype != torch.int64 or offset.numel() != 1 or offset.device != logits.device:
        raise ValueError("offset must be a one-element int64 tensor on the logits' device")
    out = torch.empty(B, 1, device=logits.device, dtype=torch.int64)
    _hip.check(_hip.lib().dw_sample_tokens(_hip.ptr(logits), _hip.dtype_code(logits), _hip.ptr(out), _hip.ptr(offset),
                                           B, V, logits.stride(0), 1.0 / float(temperature), int(top_k or 0),
                                           float(top_p), int(seed) & (2**64 - 1), _hip.stream()), "sample_tokens")
    offset.add_(1)  # same stream: a replayed graph draws fresh numbers
    return out


def sample_tokens(logits, temperature, top_k=0, top_p=1.0, generator=None, seed=None, offset=None):
    """One token per row of ``[B, V]`` logits -> int64 ``[B, 1]``.

    GPU tensor and ``seed`` given: the fused kernel.  Gumbel-max over the kept
    set with counter-based random numbers keyed by ``(seed, offset, row,
    token)``; ``offset`` is a one-element int64 device tensor that the kernel
    reads and this op advances by 1 afterwards.  The same logits, seed and
    offset give the same tokens on every run, eager or graph-replayed.

    Otherwise: ``keep_mask``, masked softmax, ``torch.multinomial(generator)``."""
    if temperature <= 0:
        return logits.argmax(-1, keepdim=True)
    if _hip.use_hip(logits) and seed is not None:
        return _sample_hip(logits, temperature, top_k, top_p, seed, offset)
    z = logits.float() / temperature
    z = z.masked_fill(~keep_mask(logits, temperature, top_k, top_p), float("-inf"))
    return torch.multinomial(z.softmax(-1), 1, generator=generator)
