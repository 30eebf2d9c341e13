"""Weight-streaming GEMM for decode (``csrc/kernels/skinny_gemm.hip``,
``docs/rl_fp8_rollouts.md``).

``skinny_linear``: ``y = (x @ w.T) * scale`` for a handful of rows of ``x``
(``M <= 64``: one decode step of an RL rollout), with ``w`` either bf16 or
OCP e4m3 codes plus one fp32 scale per output row.  ``quantize_rows_e4m3``
makes such a copy of a bf16 weight.  Both are forward only (rollouts run
under ``no_grad``); their torch forms below define the semantics, run for CPU
tensors and are the reference of the GPU tests.
"""

import functools

import torch
import torch.nn.functional as F

from . import _hip

E4M3_MAX = 448.0
MAX_ROWS = 64


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


def skinny_linear_ref(x, w, scale=None):
    """The defining expression.  bf16 / fp32 weights without a scale are
    ``F.linear`` itself; otherwise fp32 math, one rounding to ``x``'s dtype
    (bf16 in the decode step)."""
    if scale is None and w.dtype == x.dtype:
        return F.linear(x, w)
    y = x.float() @ w.float().t()
    if scale is not None:
        y = y * scale
    return y.to(x.dtype)


@functools.lru_cache(maxsize=None)
def _plan(M: int, N: int, K: int, fp8: bool, splits: int) -> int:
    """The number of K slices the launcher runs for this call (its own rule:
    ``dw_skinny_gemm_plan``); cached, so a decode step asks once per shape."""
    return int(_hip.lib().dw_skinny_gemm_plan(M, N, K, int(fp8), int(splits)))


def workspace_floats(M: int, N: int, K: int, fp8: bool, splits: int = 0) -> int:
    """fp32 elements of split-K scratch ``skinny_linear`` needs for this
    shape (0: a single slice, none)."""
    s = _plan(int(M), int(N), int(K), bool(fp8), int(splits))
    return s * M * N if s > 1 else 0


def skinny_linear(x, w, scale=None, splits: int = 0, workspace=None):
    """``x`` [..., K] bf16, ``w`` [N, K] bf16 or float8_e4m3fn, ``scale``
    fp32 [N] or None -> bf16 [..., N] = ``((x @ w.T) * scale)``, fp32
    accumulation, one rounding.

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
    N, K = w.shape
    if x.shape[-1] != K:
        raise ValueError(f"skinny_linear: x [..., {x.shape[-1]}] does not match w [{N}, {K}]")
    if scale is not None and (scale.shape != (N,) or scale.dtype != torch.float32):
        raise ValueError(f"skinny_linear: scale must be float32 [{N}], got {scale.dtype} {tuple(scale.shape)}")
    M = x.numel() // K if K else 0
    fp8 = w.dtype == torch.float8_e4m3fn
    if not (_hip.use_hip(x) and x.dtype == torch.bfloat16 and (fp8 or w.dtype == torch.bfloat16)
            and 1 <= M <= MAX_ROWS and K % 16 == 0 and w.is_contiguous() and w.data_ptr() % 16 == 0
            and w.device == x.device):
        return skinny_linear_ref(x, w, scale)
    x2 = x.reshape(M, K)
    if x2.stride(1) != 1 or (M > 1 and (x2.stride(0) % 8 or x2.stride(0) < K)) or x2.data_ptr() % 16:
        x2 = x2.contiguous()
    ldx = x2.stride(0) if M > 1 else K
    if scale is not None:
        scale = scale.contiguous()
    need = workspace_floats(M, N, K, fp8, splits)
    ws = None
    if need:
        ws = workspace
        if ws is None:
            ws = _hip.splitk_workspace(need, x.device)
        elif ws.dtype != torch.float32 or ws.numel() < need or ws.device != x.device or not ws.is_contiguous():
            raise ValueError(f"skinny_linear: workspace must be contiguous float32 with >= {need} elements on "
                             f"{x.device}")
    y = torch.empty(M, N, device=x.device, dtype=torch.bfloat16)
    _hip.check(_hip.lib().dw_skinny_gemm(_hip.ptr(x2), ldx, _hip.ptr(w), int(fp8), _hip.ptr(scale), _hip.ptr(y),
                                         _hip.ptr(ws), ws.numel() if ws is not None else 0, M, N, K, int(splits),
                                         _hip.stream()), "skinny_gemm")
    return y.view(*x.shape[:-1], N)
