"""Fused MoE token path: top-k router, expert sort, dispatch / combine
(``csrc/kernels/moe_route.hip``, ``csrc/kernels/moe_dispatch.hip``).

The pieces ``parallel/moe.py`` strings together around the experts:

* ``topk_route``: softmax + top-k + renormalisation + load-balance / z loss in
  one pass over the logits, with its own one-launch backward;
* ``sort_by_expert``: stable counting sort of the flat top-k assignment;
* ``moe_dispatch``: rows gathered into expert-grouped order -- the backward is a
  k-way row sum through the inverse permutation (no float atomics);
* ``moe_combine``: weighted k-way row sum back to token order -- the backward
  gathers ``w * dout`` and reduces ``dw`` in the same pass.

Nothing reads the device: the number of valid grouped rows (``n - counts[E]``
when the capacity path uses its sentinel bucket ``E``) stays in ``counts``.
No float atomics anywhere, so the gradients are bit-reproducible.

Tie rule of the router: the arg-max runs over the logits and on equal values
the lowest expert index wins.  Limits of the kernels: E <= 256, k <= 8 for the
router; at most 1025 buckets for the sort; bf16 rows with H % 8 == 0 (16-byte
vectors) for dispatch / combine.  CPU tensors (and rows the kernels do not
take) run the equivalent torch math.

Parity: reference ``atorch/modules/moe/grouped_gemm_moe.py`` (megablocks
``ops.sort`` / ``histogram`` / ``gather`` / ``scatter``) and
``topk_gating.py``.
"""

from typing import Optional, Tuple

import torch

from . import _hip

ROUTE_MAX_EXPERTS = 256
ROUTE_MAX_K = 8
SORT_MAX_BUCKETS = 1025


def route_kernel_takes(logits: torch.Tensor, k: int) -> bool:
    E = logits.shape[-1]
    return (_hip.use_hip(logits) and logits.dtype in (torch.float32, torch.bfloat16)
            and E <= ROUTE_MAX_EXPERTS and 1 <= k <= min(ROUTE_MAX_K, E) and logits.numel() > 0)


def rows_kernel_takes(x: torch.Tensor) -> bool:
    return _hip.use_hip(x) and x.dtype == torch.bfloat16 and x.dim() == 2 and x.shape[-1] % 8 == 0 \
        and x.shape[-1] >= 8


# --------------------------------------------------------------------------- router


def _route_torch(logits, k, norm_topk, aux_loss_coef, z_loss_coef):
    E = logits.shape[-1]
    lf = logits if logits.dtype == torch.float64 else logits.float()
    probs = lf.softmax(-1)
    # ties: lowest expert index first (a stable sort; torch.topk leaves it open)
    idx = torch.sort(lf, dim=-1, descending=True, stable=True).indices[..., :k]
    w = probs.gather(-1, idx)
    if norm_topk:
        w = w / w.sum(-1, keepdim=True)
    counts = torch.bincount(idx.reshape(-1), minlength=E)
    frac = counts.to(probs.dtype) / idx.numel()
    aux = E * (frac * probs.mean(0)).sum() * aux_loss_coef
    z = torch.logsumexp(lf, -1).square().mean() * z_loss_coef
    return w, idx, aux + z, counts


def route_forward(logits, k, norm_topk=True, aux_loss_coef=1e-2, z_loss_coef=1e-3):
    """The router kernel's raw outputs (no autograd): ``w`` [T, k], ``idx``
    [T, k], ``lse`` [T], ``counts`` [E], ``psum`` [E] (= sum_t p[t, e]) and
    ``stats`` = (loss, sum_t lse^2)."""
    x = logits.contiguous()
    T, E = x.shape
    dev = x.device
    L = _hip.lib()
    w = torch.empty(T, k, device=dev, dtype=torch.float32)
    idx = torch.empty(T, k, device=dev, dtype=torch.int64)
    lse = torch.empty(T, device=dev, dtype=torch.float32)
    counts = torch.empty(E, device=dev, dtype=torch.int64)
    psum = torch.empty(E, device=dev, dtype=torch.float32)
    stats = torch.empty(2, device=dev, dtype=torch.float32)
    ws = torch.empty(int(L.dw_moe_route_ws_floats(T)), device=dev, dtype=torch.float32)
    _hip.check(L.dw_moe_route_fwd(_hip.ptr(x), _hip.dtype_code(x), _hip.ptr(w), _hip.ptr(idx), _hip.ptr(lse),
                                  _hip.ptr(counts), _hip.ptr(psum), _hip.ptr(stats), _hip.ptr(ws), T, E, k,
                                  int(norm_topk), float(aux_loss_coef), float(z_loss_coef), _hip.stream()),
               "moe_route_fwd")
    return dict(x=x, w=w, idx=idx, lse=lse, counts=counts, psum=psum, stats=stats)


class _RouteFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, k, norm_topk, aux_loss_coef, z_loss_coef):
        r = route_forward(logits, k, norm_topk, aux_loss_coef, z_loss_coef)
        ctx.save_for_backward(r["x"], r["lse"], r["idx"], r["w"], r["counts"])
        ctx.meta = (k, int(norm_topk), float(aux_loss_coef), float(z_loss_coef))
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(r["idx"], r["counts"])
        return r["w"], r["idx"], r["stats"][0], r["counts"]

    @staticmethod
    def backward(ctx, gw, _gidx, gloss, _gcounts):
        x, lse, idx, w, counts = ctx.saved_tensors
        k, norm, a, c = ctx.meta
        T, E = x.shape
        if gw is None and gloss is None:
            return None, None, None, None, None
        if gw is not None:
            gw = gw.contiguous().float()
        if gloss is not None:
            gloss = gloss.contiguous().float()
        dx = torch.empty_like(x)
        _hip.check(_hip.lib().dw_moe_route_bwd(_hip.ptr(x), _hip.dtype_code(x), _hip.ptr(lse), _hip.ptr(idx),
                                               _hip.ptr(w), _hip.ptr(gw), _hip.ptr(gloss), _hip.ptr(counts),
                                               _hip.ptr(dx), T, E, k, norm, a, c, _hip.stream()), "moe_route_bwd")
        return dx, None, None, None, None


def topk_route(logits: torch.Tensor, k: int, norm_topk: bool = True, aux_loss_coef: float = 1e-2,
               z_loss_coef: float = 1e-3) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """Router of a top-k MoE layer over ``logits`` [T, E].

    Returns ``(w, idx, loss, counts)``: the fp32 weights [T, k] of the
    selected experts (softmax probabilities, renormalised over the selected
    set when ``norm_topk``), their indices [T, k] (int64; on equal logits the
    lowest index wins), the scalar ``aux_loss_coef * E * sum_e f_e * mean_t
    p[t, e] + z_loss_coef * mean_t lse^2`` and the per-expert assignment
    counts [E] (int64).  Differentiable in ``logits`` through ``w`` and
    ``loss``."""
    assert logits.dim() == 2, "logits: [tokens, experts]"
    if route_kernel_takes(logits, k):
        return _RouteFn.apply(logits, int(k), bool(norm_topk), aux_loss_coef, z_loss_coef)
    return _route_torch(logits, k, norm_topk, aux_loss_coef, z_loss_coef)


# --------------------------------------------------------------------------- sort


def sort_by_expert(idx: torch.Tensor, num_buckets: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Stable sort of the flat assignment ``idx`` (values in [0, num_buckets)).

    Returns ``(order, pos, counts)``: ``order`` (int32 [n]) maps a grouped row
    to its flat assignment and equals ``argsort(idx.flatten(), stable=True)``,
    ``pos`` (int32 [n]) is its inverse, ``counts`` (int64 [num_buckets]) the
    bucket sizes."""
    flat = idx.reshape(-1)
    n = flat.numel()
    if _hip.use_hip(flat) and 0 < n and num_buckets <= SORT_MAX_BUCKETS:
        flat = flat.to(torch.int64).contiguous()
        L = _hip.lib()
        dev = flat.device
        order = torch.empty(n, device=dev, dtype=torch.int32)
        pos = torch.empty(n, device=dev, dtype=torch.int32)
        counts = torch.empty(num_buckets, device=dev, dtype=torch.int64)
        ws = torch.empty(int(L.dw_moe_sort_ws_size(n, num_buckets)), device=dev, dtype=torch.int32)
        _hip.check(L.dw_moe_sort(_hip.ptr(flat), n, num_buckets, _hip.ptr(counts), _hip.ptr(order), _hip.ptr(pos),
                                 _hip.ptr(ws), _hip.stream()), "moe_sort")
        return order, pos, counts
    order = torch.argsort(flat, stable=True)
    pos = torch.empty_like(order).scatter_(0, order, torch.arange(n, device=flat.device))
    counts = torch.bincount(flat, minlength=num_buckets)
    return order.to(torch.int32), pos.to(torch.int32), counts


# --------------------------------------------------------------------------- dispatch / combine


def _sentinel(counts, num_experts):
    """(counts pointer source, sentinel bucket) of the device-side n_valid, or
    (None, 0) when every grouped row is valid."""
    if counts is not None and num_experts is not None and counts.numel() > num_experts:
        return counts, int(num_experts)
    return None, 0


def _valid_rows(n, counts, num_experts, device):
    """[n] bool: grouped row r < n_valid (torch path; no host read)."""
    c, s = _sentinel(counts, num_experts)
    if c is None:
        return None
    return torch.arange(n, device=device) < (n - c[s])


def _gather(src, order, scale, y, dw, counts, sentinel, n_rows, k):
    n, H = order.numel(), src.shape[-1]
    out = torch.empty(n_rows, H, device=src.device, dtype=src.dtype)
    _hip.check(_hip.lib().dw_moe_gather_rows(_hip.ptr(src), _hip.ptr(out), _hip.ptr(order), _hip.ptr(scale),
                                             _hip.ptr(y), _hip.ptr(dw), _hip.ptr(counts), sentinel, n_rows, n, k,
                                             H, _hip.stream()), "moe_gather_rows")
    return out


def _ksum(src, pos, scale, counts, sentinel, T, k):
    H = src.shape[-1]
    out = torch.empty(T, H, device=src.device, dtype=src.dtype)
    _hip.check(_hip.lib().dw_moe_ksum_rows(_hip.ptr(src), _hip.ptr(out), _hip.ptr(pos), _hip.ptr(scale),
                                           _hip.ptr(counts), sentinel, T, src.shape[0], k, H, _hip.stream()),
               "moe_ksum_rows")
    return out


def _i32(t):
    return t.to(torch.int32).contiguous()


class _DispatchFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, order, pos, k, counts, sentinel):
        ctx.save_for_backward(pos, counts)
        ctx.meta = (k, sentinel, x.shape[0])
        return _gather(x.contiguous(), order, None, None, None, counts, sentinel, order.numel(), k)

    @staticmethod
    def backward(ctx, g):
        pos, counts = ctx.saved_tensors
        k, sentinel, T = ctx.meta
        return _ksum(g.contiguous(), pos, None, counts, sentinel, T, k), None, None, None, None, None


class _CombineFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, w, order, pos, k, counts, sentinel):
        y = y.contiguous()
        w32 = w.contiguous().float()
        ctx.save_for_backward(y, w32, order, pos, counts)
        ctx.meta = (k, sentinel, w.dtype)
        return _ksum(y, pos, w32, counts, sentinel, w.shape[0], k)

    @staticmethod
    def backward(ctx, g):
        y, w32, order, pos, counts = ctx.saved_tensors
        k, sentinel, wdtype = ctx.meta
        n, rows = order.numel(), y.shape[0]
        # grouped rows past y (an expert-parallel y ends at n_valid) are dropped assignments: dw = 0
        dw = torch.empty(n, device=y.device, dtype=torch.float32) if rows >= n else \
            torch.zeros(n, device=y.device, dtype=torch.float32)
        dy = _gather(g.contiguous(), order, w32, y, dw, counts, sentinel, min(rows, n), k)
        if rows > n:
            dy = torch.cat([dy, dy.new_zeros(rows - n, dy.shape[-1])])
        return dy, dw.view(w32.shape).to(wdtype), None, None, None, None, None


def moe_dispatch(x: torch.Tensor, order: torch.Tensor, pos: torch.Tensor, k: int,
                 counts: Optional[torch.Tensor] = None, num_experts: Optional[int] = None) -> torch.Tensor:
    """Expert-grouped rows of ``x`` [T, H]: ``out[r] = x[order[r] // k]``.

    ``order`` / ``pos`` / ``counts`` come from ``sort_by_expert``.  When
    ``counts`` has a bucket past ``num_experts`` (the capacity path's sentinel
    for dropped assignments, sorted last), those rows are zero and take no
    gradient.  Differentiable in ``x``: ``dx[t]`` is the sum of the token's k
    grouped gradient rows, in the fixed order j = 0..k-1."""
    c, s = _sentinel(counts, num_experts)
    assert order.numel() == pos.numel() == x.shape[0] * k, "order / pos: one entry per (token, choice)"
    if rows_kernel_takes(x):
        return _DispatchFn.apply(x, _i32(order), _i32(pos), int(k), c, s)
    xs = x.index_select(0, order.long() // k)
    valid = _valid_rows(order.numel(), counts, num_experts, x.device)
    if valid is not None:
        xs = torch.where(valid.unsqueeze(-1), xs, xs.new_zeros(()))
    return xs


def moe_combine(y: torch.Tensor, w: torch.Tensor, order: torch.Tensor, pos: torch.Tensor, k: int,
                counts: Optional[torch.Tensor] = None, num_experts: Optional[int] = None) -> torch.Tensor:
    """Token-order output of the experts: ``out[t] = sum_j w[t, j] * y[pos[t *
    k + j]]`` over the token's assignments that were not dropped.

    ``y``: expert-grouped rows [>= n_valid, H]; rows at or past ``n_valid``
    (the sentinel bucket) are never read and may hold anything.  The kernel
    accumulates in fp32 and rounds once.  Differentiable in ``y`` and ``w``
    (``dw`` of a dropped assignment is 0)."""
    c, s = _sentinel(counts, num_experts)
    T = w.shape[0]
    n = order.numel()
    assert tuple(w.shape) == (T, k) and n == pos.numel() == T * k, "w: [tokens, k]; order / pos: one entry each"
    if rows_kernel_takes(y):
        return _CombineFn.apply(y, w, _i32(order), _i32(pos), int(k), c, s)
    if y.shape[0] < n:
        y = torch.cat([y, y.new_zeros(n - y.shape[0], y.shape[-1])])
    valid = _valid_rows(n, counts, num_experts, y.device)
    if valid is not None:
        y = torch.where(valid.unsqueeze(-1), y[:n], y.new_zeros(()))
    out = torch.zeros(n, y.shape[-1], dtype=y.dtype, device=y.device).index_copy(0, order.long(), y[:n])
    return (out.view(T, k, -1) * w.to(y.dtype).unsqueeze(-1)).sum(1)
