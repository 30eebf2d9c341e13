"""Weight-streaming GEMM for decode (``csrc/kernels/skinny_gemm.hip``,
``docs/rl_fp8_rollouts.md``).

``skinny_linear``: ``y = (x @ w.T) * scale`` for a handful of rows of ``x``
(``M <= 64``: one decode step of an RL rollout), with ``w`` either bf16 or
OCP e4m3 codes plus one fp32 scale per output row.  ``quantize_rows_e4m3``
makes such a copy of a bf16 weight.  A third form is OCP MXFP4
(``docs/rl_mxfp4_rollouts.md``): ``w`` uint8 [N, K/2] e2m1 codes, two per
byte, with ``scale`` uint8 [N, K/32] e8m0 block scales, made by
``quantize_rows_mxfp4`` and read back by ``dequantize_mxfp4``.  All are
forward only (rollouts run under ``no_grad``); their torch forms below define
the semantics, run for CPU tensors and are the reference of the GPU tests.
"""

import functools

import torch
import torch.nn.functional as F

from . import _hip

E4M3_MAX = 448.0
MAX_ROWS = 64
MX_BLOCK = 32
E2M1_VALUES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
_E2M1_MIDPOINTS = (0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0)
_FORMATS = {False: 0, "bf16": 0, True: 1, "fp8": 1, "mxfp4": 2}


def _quantize_ref(w):
    wf = w.float()
    amax = wf.abs().amax(dim=1)
    scale = torch.where(amax > 0, amax / E4M3_MAX, torch.ones_like(amax))
    codes = (wf / scale[:, None]).clamp(-E4M3_MAX, E4M3_MAX).to(torch.float8_e4m3fn)
    return codes, scale


def quantize_rows_e4m3(w, out=None):
    """``w`` [N, K] -> ``(codes float8_e4m3fn [N, K], scale fp32 [N])`` with
    ``scale[n] = amax_n / 448`` (1 for an all-zero row) and ``code =
    e4m3(clamp(w / scale, +-448))``, so ``w ~= codes.float() * scale[:, None]``.

    ``out = (codes, scale)``: contiguous buffers of that shape and dtype that
    are refilled in place (and returned).  A contiguous bf16 GPU weight with
    ``K % 8 == 0`` runs the HIP quantiser, one launch; anything else runs the
    torch expression above."""
    if w.dim() != 2:
        raise ValueError(f"quantize_rows_e4m3 expects a [N, K] weight, got {tuple(w.shape)}")
    N, K = w.shape
    if out is None:
        codes = torch.empty(N, K, device=w.device, dtype=torch.float8_e4m3fn)
        scale = torch.empty(N, device=w.device, dtype=torch.float32)
    else:
        codes, scale = out
        if (codes.shape != (N, K) or codes.dtype != torch.float8_e4m3fn or not codes.is_contiguous()
                or scale.shape != (N,) or scale.dtype != torch.float32 or not scale.is_contiguous()
                or codes.device != w.device or scale.device != w.device):
            raise ValueError(f"quantize_rows_e4m3: out must be contiguous (float8_e4m3fn [{N}, {K}], float32 [{N}]) "
                             f"on {w.device}")
    if (_hip.use_hip(w) and w.dtype == torch.bfloat16 and w.is_contiguous() and K % 8 == 0 and N > 0
            and w.data_ptr() % 16 == 0 and codes.data_ptr() % 8 == 0):
        _hip.check(_hip.lib().dw_quant_rows_e4m3(_hip.ptr(w), _hip.ptr(codes), _hip.ptr(scale), N, K,
                                                 _hip.stream()), "quant_rows_e4m3")
    else:
        c, s = _quantize_ref(w)
        codes.copy_(c)
        scale.copy_(s)
    return codes, scale


def _check_mx_pair(what, N, K, codes, scale, device=None):
    """``codes`` uint8 [N, K/2] and ``scale`` uint8 [N, K/32], contiguous."""
    if (codes.shape != (N, K // 2) or codes.dtype != torch.uint8 or not codes.is_contiguous()
            or scale.shape != (N, K // MX_BLOCK) or scale.dtype != torch.uint8 or not scale.is_contiguous()
            or (device is not None and (codes.device != device or scale.device != device))):
        raise ValueError(f"{what} must be contiguous (uint8 [{N}, {K // 2}], uint8 [{N}, {K // MX_BLOCK}])"
                         + (f" on {device}" if device is not None else "")
                         + f", got {codes.dtype} {tuple(codes.shape)}, {scale.dtype} {tuple(scale.shape)}")


def dequantize_mxfp4(codes, scale):
    """``codes`` uint8 [N, K/2] (byte j: element 2j in the low nibble, 2j + 1
    in the high one; nibble = sign << 3 | e2m1), ``scale`` uint8 [N, K/32]
    (e8m0: ``2^(code - 127)``) -> fp32 [N, K]."""
    if codes.dim() != 2 or (2 * codes.shape[1]) % MX_BLOCK:
        raise ValueError(f"dequantize_mxfp4 expects uint8 [N, K/2] codes with K % {MX_BLOCK} == 0, got "
                         f"{tuple(codes.shape)}")
    N, K = codes.shape[0], 2 * codes.shape[1]
    _check_mx_pair("dequantize_mxfp4: (codes, scale)", N, K, codes, scale)
    table = torch.tensor(E2M1_VALUES + tuple(-v for v in E2M1_VALUES), device=codes.device)
    nib = torch.stack((codes & 15, codes >> 4), dim=-1).view(N, K).long()
    block = torch.exp2(scale.float() - 127.0)
    return (table[nib].view(N, K // MX_BLOCK, MX_BLOCK) * block[:, :, None]).view(N, K)


def _quantize_mx_ref(w):
    N, K = w.shape
    wf = w.float().view(N, K // MX_BLOCK, MX_BLOCK)
    amax = wf.abs().amax(dim=2)
    # floor(log2(amax)) + 127 is amax's fp32 exponent field; OCP: shared exponent = that - emax(e2m1) = - 2
    field = (amax.view(torch.int32) >> 23) & 0xFF
    code = torch.where(amax > 0, (field - 2).clamp(1, 254), torch.full_like(field, 127))
    a = wf.abs() * torch.exp2(127.0 - code.float())[:, :, None]   # a power of two: exact
    mids = torch.tensor(_E2M1_MIDPOINTS, device=w.device)
    lo, hi = torch.bucketize(a, mids), torch.bucketize(a, mids, right=True)   # they differ on a midpoint
    mag = torch.where((hi != lo) & (lo % 2 == 1), hi, lo)                     # ... which goes to the even code
    nib = (mag | ((wf < 0).long() << 3)).view(N, K // 2, 2)
    return (nib[..., 0] | (nib[..., 1] << 4)).to(torch.uint8), code.to(torch.uint8)


def quantize_rows_mxfp4(w, out=None):
    """``w`` [N, K], ``K % 32 == 0`` -> ``(codes uint8 [N, K/2], scale uint8
    [N, K/32])``, the layout of ``dequantize_mxfp4``.  Per block of 32 along K
    (the OCP MX rule): ``scale = clamp(floor(log2(amax)) - 2 + 127, 1, 254)``
    (127 for an all-zero block), element = ``w * 2^(127 - scale)`` rounded to
    the nearest of ``E2M1_VALUES``, ties to the even code, saturated at 6.  So
    ``|deq - w| <= |w| / 4 + 2^(scale - 129)``.

    ``out = (codes, scale)``: contiguous buffers of that shape and dtype that
    are refilled in place (and returned).  A contiguous bf16 GPU weight runs
    the HIP quantiser, one launch; anything else the torch expression above."""
    if w.dim() != 2:
        raise ValueError(f"quantize_rows_mxfp4 expects a [N, K] weight, got {tuple(w.shape)}")
    N, K = w.shape
    if K % MX_BLOCK:
        raise ValueError(f"quantize_rows_mxfp4: K = {K} is not a multiple of the MX block of {MX_BLOCK}")
    if out is None:
        codes = torch.empty(N, K // 2, device=w.device, dtype=torch.uint8)
        scale = torch.empty(N, K // MX_BLOCK, device=w.device, dtype=torch.uint8)
    else:
        codes, scale = out
        _check_mx_pair("quantize_rows_mxfp4: out", N, K, codes, scale, w.device)
    if (_hip.use_hip(w) and w.dtype == torch.bfloat16 and w.is_contiguous() and N > 0 and K > 0
            and w.data_ptr() % 16 == 0 and codes.data_ptr() % 4 == 0):
        _hip.check(_hip.lib().dw_quant_rows_mxfp4(_hip.ptr(w), _hip.ptr(codes), _hip.ptr(scale), N, K,
                                                  _hip.stream()), "quant_rows_mxfp4")
    else:
        c, s = _quantize_mx_ref(w)
        codes.copy_(c)
        scale.copy_(s)
    return codes, scale


def skinny_linear_ref(x, w, scale=None):
    """The defining expression.  bf16 / fp32 weights without a scale are
    ``F.linear`` itself; otherwise fp32 math, one rounding to ``x``'s dtype
    (bf16 in the decode step).  uint8 ``w`` and ``scale`` are the MXFP4 form:
    ``x @ dequantize_mxfp4(w, scale).T``."""
    if scale is None and w.dtype == x.dtype:
        return F.linear(x, w)
    if w.dtype == torch.uint8:
        return (x.float() @ dequantize_mxfp4(w, scale).t()).to(x.dtype)
    y = x.float() @ w.float().t()
    if scale is not None:
        y = y * scale
    return y.to(x.dtype)


@functools.lru_cache(maxsize=None)
def _plan(M: int, N: int, K: int, fmt: int, splits: int) -> int:
    """The number of K slices the launcher runs for this call (its own rule:
    ``dw_skinny_gemm_plan``); cached per format code, so a decode step asks
    once per shape."""
    return int(_hip.lib().dw_skinny_gemm_plan(M, N, K, fmt, int(splits)))


def workspace_floats(M: int, N: int, K: int, fp8=False, splits: int = 0) -> int:
    """fp32 elements of split-K scratch ``skinny_linear`` needs for this
    shape (0: a single slice, none).  ``fp8``: the weight format, ``False`` /
    ``"bf16"``, ``True`` / ``"fp8"`` or ``"mxfp4"``."""
    fmt = _FORMATS.get(fp8 if isinstance(fp8, str) else bool(fp8))
    if fmt is None:
        raise ValueError(f"workspace_floats: format must be one of {list(_FORMATS)}, got {fp8!r}")
    s = _plan(int(M), int(N), int(K), fmt, int(splits))
    return s * M * N if s > 1 else 0


def skinny_linear(x, w, scale=None, splits: int = 0, workspace=None):
    """``x`` [..., K] bf16, ``w`` [N, K] bf16 or float8_e4m3fn, ``scale``
    fp32 [N] or None -> bf16 [..., N] = ``((x @ w.T) * scale)``, fp32
    accumulation, one rounding.  ``w`` uint8 [N, K/2] with ``scale`` uint8
    [N, K/32] is the MXFP4 form: ``x @ dequantize_mxfp4(w, scale).T``, the
    block scales applied as the codes are decoded (k chunks of 128).

    The HIP kernel takes GPU calls with bf16 ``x``, ``1 <= M <= 64`` rows
    (``M`` = the product of the leading dims), ``K % 16 == 0`` and a
    contiguous 16-byte aligned ``w``; ``x`` may be a row-strided view (last
    dim contiguous, row stride a multiple of 8), any other layout is copied.
    ``splits``: the number of K slices whose fp32 partial sums are added in a
    fixed order (0: the kernel's choice, a function of ``(M, N, K)``; a larger
    value than there are 32-deep (bf16) / 64-deep (e4m3) k chunks is clamped).
    Results are bit-reproducible for a given ``splits``.
    ``workspace``: the caller's fp32 scratch of at least ``workspace_floats``
    elements for the partial sums; by default one buffer per (device, stream)
    that grows on demand (``_hip.splitk_workspace``).  A caller that records
    graphs on streams of its own passes its buffer, so that no capture
    allocates.

    Outside that contract (``M > 64``, ``K % 16 != 0``, ``x`` not bf16, a
    non-contiguous ``w``, CPU tensors) the call computes ``skinny_linear_ref``
    with torch: the same function, not the streaming kernel."""
    mx = w.dtype == torch.uint8
    N, K = w.shape[0], (2 if mx else 1) * w.shape[1]
    if x.shape[-1] != K:
        raise ValueError(f"skinny_linear: x [..., {x.shape[-1]}] does not match w [{N}, {K}]")
    if mx:
        if (scale is None or scale.dtype != torch.uint8 or K % MX_BLOCK or scale.shape != (N, K // MX_BLOCK)
                or scale.device != w.device):
            got = "None" if scale is None else f"{scale.dtype} {tuple(scale.shape)}"
            raise ValueError(f"skinny_linear: uint8 w [{N}, {K // 2}] is MXFP4 codes (K % {MX_BLOCK} == 0) and needs "
                             f"scale uint8 [{N}, {K // MX_BLOCK}], got {got}")
    elif scale is not None and (scale.shape != (N,) or scale.dtype != torch.float32):
        raise ValueError(f"skinny_linear: scale must be float32 [{N}], got {scale.dtype} {tuple(scale.shape)}")
    M = x.numel() // K if K else 0
    fp8 = w.dtype == torch.float8_e4m3fn
    fmt = "mxfp4" if mx else fp8
    if not (_hip.use_hip(x) and x.dtype == torch.bfloat16 and (fp8 or mx or w.dtype == torch.bfloat16)
            and 1 <= M <= MAX_ROWS and K % 16 == 0 and w.is_contiguous() and w.data_ptr() % 16 == 0
            and w.device == x.device):
        if mx:
            scale = scale.contiguous()
            w = w.contiguous()
        return skinny_linear_ref(x, w, scale)
    x2 = x.reshape(M, K)
    if x2.stride(1) != 1 or (M > 1 and (x2.stride(0) % 8 or x2.stride(0) < K)) or x2.data_ptr() % 16:
        x2 = x2.contiguous()
    ldx = x2.stride(0) if M > 1 else K
    if scale is not None:
        scale = scale.contiguous()
    need = workspace_floats(M, N, K, fmt, splits)
    ws = None
    if need:
        ws = workspace
        if ws is None:
            ws = _hip.splitk_workspace(need, x.device)
        elif ws.dtype != torch.float32 or ws.numel() < need or ws.device != x.device or not ws.is_contiguous():
            raise ValueError(f"skinny_linear: workspace must be contiguous float32 with >= {need} elements on "
                             f"{x.device}")
    y = torch.empty(M, N, device=x.device, dtype=torch.bfloat16)
    _hip.check(_hip.lib().dw_skinny_gemm(_hip.ptr(x2), ldx, _hip.ptr(w), _FORMATS[fmt], _hip.ptr(scale), _hip.ptr(y),
                                         _hip.ptr(ws), ws.numel() if ws is not None else 0, M, N, K, int(splits),
                                         _hip.stream()), "skinny_gemm")
    return y.view(*x.shape[:-1], N)
