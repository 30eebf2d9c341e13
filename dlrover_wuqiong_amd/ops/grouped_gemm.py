"""Grouped (per-expert) linear layers on one HIP launch per GEMM
(``csrc/kernels/grouped_gemm.hip``).

``grouped_linear(x, w, offs)``: rows ``[offs[e], offs[e+1])`` of ``x`` [T, K]
go through expert ``e``'s weight ``w[e]`` [N, K] (nn.Linear layout) ->
[T, N].  ``offs`` ([E+1] int32) stays on the device, so an MoE layer never
synchronises with the host to read its per-expert token counts.  Backward:
dX by the NN form, dW by the TN form (one launch each, reduction over each
group's rows).

``grouped_swiglu_linear(x, w1, w3, offs)``: the gate / up half of a SwiGLU
expert FFN, ``silu(x w1[e]^T) * (x w3[e]^T)``, in one launch that loads each
``x`` tile once and applies the activation in the GEMM epilogue; it keeps
only the packed pre-activations ``gu`` [T, 2F] for the backward, whose dgrad
sums both weights' contributions in one accumulation (docs/moe_experts.md).

CPU tensors run the per-expert PyTorch loop (reference math / gloo path).

Parity: ATorch grouped-GEMM experts (atorch/atorch/modules/moe/
grouped_gemm_moe.py:46-112).
"""

from typing import List, Union

import torch
import torch.nn.functional as F

from . import _hip

MODE_NT, MODE_NN, MODE_TN = 0, 1, 2


def offsets_from_counts(counts: Union[torch.Tensor, List[int]], device) -> torch.Tensor:
    """[E] counts (device tensor or host list) -> [E+1] int32 offsets on ``device``."""
    if not torch.is_tensor(counts):
        counts = torch.tensor(list(counts), dtype=torch.int64)
    c = counts.to(device=device, dtype=torch.int64, non_blocking=True)
    offs = torch.zeros(c.numel() + 1, dtype=torch.int32, device=device)
    torch.cumsum(c, 0, out=offs[1:])
    return offs


def _launch(mode, A, B, C, offs, E, T, M, Nout, R, lda, ldb, ldc, b_es, c_es):
    _hip.check(_hip.lib().dw_grouped_gemm(mode, _hip.ptr(A), _hip.ptr(B), _hip.ptr(C), _hip.ptr(offs), E, T, M, Nout,
                                          R, lda, ldb, ldc, b_es, c_es, _hip.stream()), "grouped_gemm")


def _check_shapes(x, w):
    T, K = x.shape
    E, N, K2 = w.shape
    if K2 != K:
        raise ValueError(f"grouped_linear: x [{T}, {K}] vs w [{E}, {N}, {K2}]")
    if K % 8 or N % 8:
        raise _hip.HipKernelError(f"grouped GEMM needs K and N divisible by 8 (got K={K}, N={N})")
    return T, K, E, N


class _GroupedLinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, offs):
        _hip.require_bf16(x, w)
        x, w = x.contiguous(), w.contiguous()
        T, K, E, N = _check_shapes(x, w)
        y = torch.empty(T, N, device=x.device, dtype=x.dtype)
        if T > 0:
            _launch(MODE_NT, x, w, y, offs, E, T, 0, N, K, K, K, N, N * K, 0)
        ctx.save_for_backward(x, w, offs)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, offs = ctx.saved_tensors
        dy = dy.contiguous().to(torch.bfloat16)
        T, K = x.shape
        E, N, _ = w.shape
        dx = dw = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            if T > 0:
                _launch(MODE_NN, dy, w, dx, offs, E, T, 0, K, N, N, K, K, N * K, 0)
        if ctx.needs_input_grad[1]:
            dw = torch.empty_like(w)
            _launch(MODE_TN, dy, x, dw, offs, E, T, N, K, 0, N, K, K, 0, N * K)
        return dx, dw, None


def grouped_linear_reference(x: torch.Tensor, w: torch.Tensor, offs: torch.Tensor) -> torch.Tensor:
    """Per-expert loop (autograd-able): the CPU path and the numerics oracle."""
    o = offs.tolist()
    outs = [F.linear(x[o[e]:o[e + 1]], w[e]) for e in range(w.shape[0])]
    y = torch.cat(outs, 0) if outs else x.new_zeros((0, w.shape[1]))
    if y.shape[0] == 0:
        y = y + 0 * w.sum()  # keep w in the graph
    return y


def grouped_linear(x: torch.Tensor, w: torch.Tensor, offs: torch.Tensor) -> torch.Tensor:
    """x [T, K] (rows grouped by expert), w [E, N, K], offs [E+1] int32 -> [T, N]."""
    if _hip.use_hip(x):
        return _GroupedLinearFn.apply(x, w, offs.to(device=x.device, dtype=torch.int32))
    return grouped_linear_reference(x, w, offs)


def _check_glu_shapes(x, w1, w3):
    T, H = x.shape
    E, F_, H2 = w1.shape
    if H2 != H or tuple(w3.shape) != tuple(w1.shape):
        raise ValueError(f"grouped_swiglu_linear: x [{T}, {H}] vs w1 {list(w1.shape)}, w3 {list(w3.shape)}")
    if H % 8 or F_ % 8:
        raise _hip.HipKernelError(f"grouped SwiGLU GEMM needs H and F divisible by 8 (got H={H}, F={F_})")
    return T, H, E, F_


def _glu_forward(x, w1, w3, offs):
    _hip.require_bf16(x, w1, w3)
    T, H, E, F_ = _check_glu_shapes(x, w1, w3)
    gu = torch.empty(T, 2 * F_, device=x.device, dtype=x.dtype)
    h = torch.empty(T, F_, device=x.device, dtype=x.dtype)
    if T > 0:
        _hip.check(_hip.lib().dw_grouped_glu_fwd(_hip.ptr(x), _hip.ptr(w1), _hip.ptr(w3), _hip.ptr(gu), _hip.ptr(h),
                                                 _hip.ptr(offs), E, T, H, F_, _hip.stream()), "grouped_glu_fwd")
    return h, gu


class _GroupedSwiGLUFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w1, w3, offs):
        x, w1, w3 = x.contiguous(), w1.contiguous(), w3.contiguous()
        h, gu = _glu_forward(x, w1, w3, offs)
        ctx.save_for_backward(x, w1, w3, offs, gu)
        return h

    @staticmethod
    def backward(ctx, dh):
        x, w1, w3, offs, gu = ctx.saved_tensors
        T, H = x.shape
        E, F_, _ = w1.shape
        need_x, need_w1, need_w3 = ctx.needs_input_grad[:3]
        dx = dw1 = dw3 = None
        if not (need_x or need_w1 or need_w3):
            return None, None, None, None
        dh = dh.contiguous().to(torch.bfloat16)
        # packed [d gate | d up]; rows past offs[E] hold whatever gu held there and are never read
        dgu = torch.empty_like(gu)
        if T > 0:
            _hip.check(_hip.lib().dw_swiglu_bwd(_hip.ptr(dh), _hip.ptr(gu), _hip.ptr(dgu), T, F_, _hip.stream()),
                       "swiglu_bwd")
        if need_x:
            dx = torch.empty_like(x)
            if T > 0:
                _hip.check(_hip.lib().dw_grouped_glu_dgrad(_hip.ptr(dgu), _hip.ptr(w1), _hip.ptr(w3), _hip.ptr(dx),
                                                           _hip.ptr(offs), E, T, H, F_, _hip.stream()),
                           "grouped_glu_dgrad")
        if need_w1:
            dw1 = torch.empty_like(w1)
            _launch(MODE_TN, dgu, x, dw1, offs, E, T, F_, H, 0, 2 * F_, H, H, 0, F_ * H)
        if need_w3:
            dw3 = torch.empty_like(w3)
            _launch(MODE_TN, dgu[:, F_:], x, dw3, offs, E, T, F_, H, 0, 2 * F_, H, H, 0, F_ * H)
        return dx, dw1, dw3, None


def grouped_swiglu_reference(x: torch.Tensor, w1: torch.Tensor, w3: torch.Tensor, offs: torch.Tensor) -> torch.Tensor:
    """Per-expert loop (autograd-able): the CPU path and the numerics oracle."""
    o = offs.tolist()
    outs = [F.silu(F.linear(x[o[e]:o[e + 1]], w1[e])) * F.linear(x[o[e]:o[e + 1]], w3[e])
            for e in range(w1.shape[0])]
    h = torch.cat(outs, 0) if outs else x.new_zeros((0, w1.shape[1]))
    if h.shape[0] == 0:
        h = h + 0 * (w1.sum() + w3.sum())  # keep the weights in the graph
    return h


def grouped_glu_forward(x: torch.Tensor, w1: torch.Tensor, w3: torch.Tensor, offs: torch.Tensor):
    """Raw fused forward (no autograd): ``(h [T, F], gu [T, 2F])`` with
    ``gu = [x w1[e]^T | x w3[e]^T]`` and ``h = silu(gu[:, :F]) * gu[:, F:]``."""
    if not _hip.use_hip(x):
        raise _hip.HipKernelError("grouped_glu_forward is the HIP kernel's entry: it needs GPU tensors")
    return _glu_forward(x.contiguous(), w1.contiguous(), w3.contiguous(),
                        offs.to(device=x.device, dtype=torch.int32))


def grouped_swiglu_linear(x: torch.Tensor, w1: torch.Tensor, w3: torch.Tensor, offs: torch.Tensor) -> torch.Tensor:
    """x [T, H] (rows grouped by expert), w1 / w3 [E, F, H], offs [E+1] int32 ->
    h [T, F] = silu(x w1[e]^T) * (x w3[e]^T).  bf16 only on the GPU, H % 8 == 0
    and F % 8 == 0."""
    if _hip.use_hip(x):
        return _GroupedSwiGLUFn.apply(x, w1, w3, offs.to(device=x.device, dtype=torch.int32))
    return grouped_swiglu_reference(x, w1, w3, offs)
