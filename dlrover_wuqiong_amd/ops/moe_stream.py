"""Weight-streaming expert FFN for the decode step of a top-k MoE layer
(``csrc/kernels/moe_stream.hip``, ``docs/rl_moe_decode.md``).

``moe_stream_mlp``: for a handful of tokens ``x`` [T, H] and the router's
``w`` / ``idx`` [T, k] (what ``ops.moe.route_forward`` / ``TopKGate`` return)

    y[t] = sum_j w[t, j] * (silu(x[t] W1[e]^T) * (x[t] W3[e]^T)) W2[e]^T,  e = idx[t, j]

read straight from the stacked expert weights ``W1`` / ``W3`` [E, F, H] and
``W2`` [E, H, F] -- bf16, or e4m3 codes with one fp32 scale per output row
(``scales``).  No sort, no dispatch copy, three launches, no host read; only
the weights of experts that were routed to are streamed.  Forward only
(rollouts run under ``no_grad``).  ``moe_stream_mlp_ref`` is the same
expression in torch: it defines the semantics, runs for CPU tensors and for
everything outside the kernel's contract, and is the reference of the tests.
"""

import functools

import torch
import torch.nn.functional as F

from . import _hip

_MAX_ROWS, _MAX_K, _MAX_SLOTS, _MAX_EXPERTS = 64, 8, 512, 256   # the kernels' limits


def moe_stream_mlp_ref(x, w, idx, w1, w3, w2, scales=None):
    """The defining expression, without a host read: every expert runs over
    all T rows and a row's result counts with the weight of its assignment to
    that expert (0 when it has none; an ``idx`` outside ``[0, E)`` is a
    dropped assignment).  fp32 math for bf16 ``x`` with ``h`` and ``y`` rounded
    once each; fp32 / fp64 ``x`` in its own precision."""
    E = w1.shape[0]
    ct = x.dtype if x.dtype in (torch.float32, torch.float64) else torch.float32
    s1, s3, s2 = scales if scales is not None else (None, None, None)
    xf = x.to(ct)
    y = torch.zeros(x.shape[0], w2.shape[1], device=x.device, dtype=ct)
    for e in range(E):
        coef = (w.to(ct) * (idx == e)).sum(1, keepdim=True)
        g, u = F.linear(xf, w1[e].to(ct)), F.linear(xf, w3[e].to(ct))
        if s1 is not None:
            g, u = g * s1[e].to(ct), u * s3[e].to(ct)
        z = F.linear((F.silu(g) * u).to(x.dtype).to(ct), w2[e].to(ct))
        if s2 is not None:
            z = z * s2[e].to(ct)
        y = y + coef * z
    return y.to(x.dtype)


@functools.lru_cache(maxsize=None)
def _plan(T: int, k: int, E: int, H: int, F_: int) -> int:
    """Slices of the down projection's K: the launcher's own rule
    (``dw_moe_stream_plan``), a function of the shapes only."""
    return int(_hip.lib().dw_moe_stream_plan(T, k, E, H, F_))


def workspace_bytes(T: int, k: int, E: int, H: int, F: int) -> int:
    """Bytes of ``moe_stream_mlp``'s workspace for this shape: ``hbuf`` bf16
    [T k, F] then the down projection's fp32 partial sums [slices, T k, H]."""
    T, k, E, H, F = int(T), int(k), int(E), int(H), int(F)
    return (T * k * F * 2 + 15) // 16 * 16 + _plan(T, k, E, H, F) * T * k * H * 4


def _kernel_takes(x, w, idx, w1, w3, w2, scales):
    if not (_hip.use_hip(x) and x.dtype == torch.bfloat16 and x.dim() == 2 and idx.dim() == 2 and w1.dim() == 3):
        return False
    T, H = x.shape
    k = idx.shape[1]
    E, F_, _ = w1.shape
    fp8 = w1.dtype == torch.float8_e4m3fn
    if not (1 <= T <= _MAX_ROWS and 1 <= k <= _MAX_K and T * k <= _MAX_SLOTS and 1 <= E <= _MAX_EXPERTS
            and H >= 16 and H % 16 == 0 and F_ >= 16 and F_ % 16 == 0):
        return False
    if not (fp8 or w1.dtype == torch.bfloat16) or w3.dtype != w1.dtype or w2.dtype != w1.dtype or fp8 != (
            scales is not None):
        return False
    if idx.dtype != torch.int64 or w.dtype != torch.float32:
        return False
    ts = (w1, w3, w2) + (tuple(scales) if fp8 else ())
    if fp8 and any(s.dtype != torch.float32 for s in scales):
        return False
    return all(t.is_contiguous() and t.data_ptr() % 16 == 0 and t.device == x.device for t in ts)


def moe_stream_mlp(x, w, idx, w1, w3, w2, scales=None, workspace=None):
    """``x`` [T, H], ``w`` fp32 [T, k], ``idx`` int64 [T, k] (a token's k
    experts distinct; a value outside ``[0, E)`` contributes 0), ``w1`` / ``w3``
    [E, F, H], ``w2`` [E, H, F] -> [T, H] in ``x``'s dtype.  ``scales = (s1,
    s3, s2)``: fp32 [E, F], [E, F], [E, H], the row scales of float8_e4m3fn
    weights (``ops.skinny_gemm.quantize_rows_e4m3`` on the [E F, H] / [E H, F]
    views).

    The HIP kernels take bf16 GPU ``x`` with ``1 <= T <= 64``, ``k <= 8``,
    ``T k <= 512``, ``E <= 256``, ``H % 16 == 0``, ``F % 16 == 0`` and
    contiguous 16-byte aligned bf16 or e4m3 weights; everything else computes
    ``moe_stream_mlp_ref`` with torch.  fp32 accumulation, ``h`` and ``y``
    rounded to bf16 once each, partial sums added in a fixed order:
    bit-reproducible for given shapes.  ``workspace``: the caller's contiguous
    uint8 buffer of at least ``workspace_bytes`` bytes (16-byte aligned) for
    ``hbuf`` and the partial sums -- a caller that records graphs passes its
    own; by default a fresh one per call."""
    if x.dim() != 2 or idx.shape != w.shape or idx.shape[0] != x.shape[0] or w1.dim() != 3 \
            or w1.shape[2] != x.shape[1] or w3.shape != w1.shape or w2.shape != (w1.shape[0], w1.shape[2], w1.shape[1]):
        raise ValueError(f"moe_stream_mlp: x {tuple(x.shape)}, w {tuple(w.shape)}, idx {tuple(idx.shape)}, w1 "
                         f"{tuple(w1.shape)}, w3 {tuple(w3.shape)}, w2 {tuple(w2.shape)} do not fit "
                         "([T, H], [T, k], [T, k], [E, F, H], [E, F, H], [E, H, F])")
    E, F_, H = w1.shape
    if scales is not None and [tuple(s.shape) for s in scales] != [(E, F_), (E, F_), (E, H)]:
        raise ValueError(f"moe_stream_mlp: scales must be (s1 [{E}, {F_}], s3 [{E}, {F_}], s2 [{E}, {H}])")
    if not _kernel_takes(x, w, idx, w1, w3, w2, scales):
        return moe_stream_mlp_ref(x, w, idx, w1, w3, w2, scales)
    T, k = idx.shape
    need = workspace_bytes(T, k, E, H, F_)
    ws = workspace
    if ws is None:
        ws = torch.empty(need, device=x.device, dtype=torch.uint8)
    elif (ws.dtype != torch.uint8 or ws.numel() < need or ws.device != x.device or not ws.is_contiguous()
          or ws.data_ptr() % 16):
        raise ValueError(f"moe_stream_mlp: workspace must be contiguous 16-byte aligned uint8 with >= {need} "
                         f"elements on {x.device}")
    x, w, idx = x.contiguous(), w.contiguous(), idx.contiguous()
    s1, s3, s2 = scales if scales is not None else (None, None, None)
    y = torch.empty(T, H, device=x.device, dtype=torch.bfloat16)
    _hip.check(_hip.lib().dw_moe_stream_mlp(_hip.ptr(x), _hip.ptr(w), _hip.ptr(idx), _hip.ptr(w1), _hip.ptr(w3),
                                            _hip.ptr(w2), _hip.ptr(s1), _hip.ptr(s3), _hip.ptr(s2),
                                            int(scales is not None), _hip.ptr(y), _hip.ptr(ws), ws.numel(), T, k, E,
                                            H, F_, _hip.stream()), "moe_stream_mlp")
    return y
