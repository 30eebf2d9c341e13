"""GPU: the fused cross-entropy kernels (``csrc/kernels/xent.hip``) against
``F.cross_entropy`` on the same bf16 values upcast to fp64.

Bounds (not taken from what the kernel gives):

* per-row loss (fp32): ``|loss - ref| <= 1e-4``.  The fast ``exp`` carries an
  argument error of about ``|x - max| * 2^-24``; at the logit ranges used here
  (``|x - max|`` up to ~70 in the peaked rows) that stays below 2e-5 on the lse.
  A ``"sum"`` of n valid rows is held to ``n * 1e-4`` (every row within its
  bound), a ``"mean"`` to 1e-4.
* dlogits (bf16): relative L2 error per row against fp64 at most twice the
  error of rounding the fp64 gradient itself to bf16 (computed in the test);
  the factor covers fp32 math and the fast ``exp``.  A row whose reference is
  exactly zero (ignored target, a single finite logit) must be exactly zero.

The one place that needs something else is said where it is used
(``_check_peak_target_row``)."""

import pytest
import torch
import torch.nn.functional as F

from dlrover_wuqiong_amd.ops import _hip
from dlrover_wuqiong_amd.ops.cross_entropy import cross_entropy

pytestmark = pytest.mark.gpu
DEV = "cuda"
T = 37
LOSS_TOL = 1e-4
NEG = float("-inf")


def _logits(shape, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (3 * torch.randn(*shape, device=DEV, generator=g)).to(torch.bfloat16)


def _targets(n, V, seed, ignore_index=-100, allowed=None):
    """n targets from ``allowed`` (default: every class) with several ignored
    entries; the first and last allowed class both appear."""
    g = torch.Generator(device=DEV).manual_seed(seed + 1)
    allowed = torch.arange(V, device=DEV) if allowed is None else allowed.to(DEV)
    t = allowed[torch.randint(0, allowed.numel(), (n,), device=DEV, generator=g)]
    if ignore_index >= 0:
        t[t == ignore_index] = allowed[allowed != ignore_index][0]
    t[0], t[1] = allowed[0], allowed[-1]
    if n > 20:
        t[3] = t[10] = t[20] = ignore_index
    else:
        t[3] = ignore_index
    return t


def _weights(shape, seed):
    g = torch.Generator(device=DEV).manual_seed(seed + 2)
    return torch.randn(*shape, device=DEV, generator=g)


def _ref(x, tgt, upstream, reduction="none", ignore_index=-100, smoothing=0.0):
    """fp64 loss and dlogits of ``upstream(loss)`` on the values of ``x``."""
    V = x.shape[-1]
    leaf = x.detach().double().requires_grad_()
    loss = F.cross_entropy(leaf.reshape(-1, V), tgt.reshape(-1), ignore_index=ignore_index,
                           label_smoothing=smoothing, reduction=reduction)
    if reduction == "none":
        loss = loss.view(tgt.shape)
    grad, = torch.autograd.grad(upstream(loss), leaf)
    return loss.detach(), grad


def _hip_run(x, tgt, upstream, **kw):
    leaf = x.detach().clone().requires_grad_()
    loss = cross_entropy(leaf, tgt, **kw)
    assert loss.dtype == torch.float32
    grad, = torch.autograd.grad(upstream(loss), leaf)
    assert grad.dtype == torch.bfloat16 and grad.shape == x.shape
    return loss.detach(), grad


def _check_loss(tag, loss, ref, tol=LOSS_TOL):
    assert loss.shape == ref.shape
    assert bool(torch.isfinite(loss).all()), loss
    err = float((loss.double() - ref).abs().max())
    print(f"[xent {tag}] max |loss - ref64| = {err:.3e} (bound {tol:.1e})")
    assert err <= tol, err
    return err


def _check_grad_rows(tag, got, ref, skip_rows=None):
    """Relative L2 per row <= 2 x the bf16 rounding floor of the fp64
    gradient; exactly-zero reference rows exactly zero."""
    V = ref.shape[-1]
    assert bool(torch.isfinite(got).all())
    g, r = got.double().reshape(-1, V), ref.reshape(-1, V)
    if skip_rows is not None:
        keep = torch.ones(g.shape[0], dtype=torch.bool, device=g.device)
        keep[skip_rows] = False
        g, r = g[keep], r[keep]
    nrm = r.norm(dim=-1)
    zero = nrm == 0
    assert bool((g[zero] == 0).all()), "rows with a zero reference gradient must be exactly zero"
    err = (g - r).norm(dim=-1)[~zero]
    floor = (r.to(torch.bfloat16).double() - r).norm(dim=-1)[~zero]
    ratio = torch.where(err > 0, err / floor, torch.zeros_like(err))
    mx = float(ratio.max()) if ratio.numel() else 0.0
    print(f"[xent {tag}] max row err / bf16 floor = {mx:.6f} (bound 2), "
          f"max row rel-L2 = {float((err / nrm[~zero]).max()) if err.numel() else 0.0:.3e}, "
          f"{int(zero.sum())} exact-zero rows")
    assert bool((err <= 2 * floor).all()), mx
    return mx


# ------------------------------------------------------------------ sizes
@pytest.mark.parametrize("V", [8, 1000, 1001, 2056, 4099, 50257])
def test_vocab_sizes_per_row_loss_and_grad(V):
    """V = 8: the whole row is one thread's chunk; 1001 / 4099 / 50257: rows
    off the 16-byte boundary plus a scalar tail; 2056: the first V at which a
    thread owns two vector chunks."""
    x = _logits((T, V), V)
    if V % 8:
        assert x[1].data_ptr() % 16 != 0
    tgt = _targets(T, V, V)
    assert int((tgt == -100).sum()) == 3 and 0 in tgt.tolist() and V - 1 in tgt.tolist()
    w = _weights((T,), V)
    loss, grad = _hip_run(x, tgt, lambda l: (l * w).sum(), reduction="none")
    rloss, rgrad = _ref(x, tgt, lambda l: (l * w.double()).sum())
    assert bool((loss[tgt == -100] == 0).all())
    _check_loss(f"V={V}", loss, rloss)
    _check_grad_rows(f"V={V}", grad, rgrad)


# ------------------------------------------------------------------ reductions
@pytest.mark.parametrize("ignore_index", [-100, 5])
@pytest.mark.parametrize("reduction", ["mean", "sum", "none"])
def test_reductions_with_upstream_gradient(reduction, ignore_index):
    V = 1000
    x = _logits((T, V), 11)
    tgt = _targets(T, V, 11, ignore_index=ignore_index)
    n_valid = int((tgt != ignore_index).sum())
    assert n_valid == T - 3
    if reduction == "none":
        w = _weights((T,), 11)
        up, rup = (lambda l: (l * w).sum()), (lambda l: (l * w.double()).sum())
    else:
        up = rup = lambda l: l * 3.0
    kw = dict(reduction=reduction, ignore_index=ignore_index)
    loss, grad = _hip_run(x, tgt, up, **kw)
    rloss, rgrad = _ref(x, tgt, rup, **kw)
    tag = f"{reduction} ignore={ignore_index}"
    _check_loss(tag, loss, rloss, LOSS_TOL * (n_valid if reduction == "sum" else 1))
    _check_grad_rows(tag, grad, rgrad)
    assert bool((grad[tgt == ignore_index] == 0).all())


def test_mean_with_every_target_ignored_is_zero():
    """The project's contract (``clamp(min=1)`` on the valid count): loss 0
    and an all-zero gradient, where torch returns NaN."""
    V = 1000
    x = _logits((T, V), 12)
    tgt = torch.full((T,), -100, device=DEV)
    loss, grad = _hip_run(x, tgt, lambda l: l * 3.0, reduction="mean")
    assert float(loss) == 0.0
    assert bool((grad == 0).all())


# ------------------------------------------------------------------ smoothing
@pytest.mark.parametrize("reduction", ["none", "mean"])
@pytest.mark.parametrize("V", [1000, 1001])
def test_label_smoothing(V, reduction):
    x = _logits((T, V), 13 + V)
    tgt = _targets(T, V, 13)
    if reduction == "none":
        w = _weights((T,), 13)
        up, rup = (lambda l: (l * w).sum()), (lambda l: (l * w.double()).sum())
    else:
        up = rup = lambda l: l * 3.0
    loss, grad = _hip_run(x, tgt, up, reduction=reduction, label_smoothing=0.1)
    rloss, rgrad = _ref(x, tgt, rup, reduction=reduction, smoothing=0.1)
    _check_loss(f"smoothing V={V} {reduction}", loss, rloss)
    _check_grad_rows(f"smoothing V={V} {reduction}", grad, rgrad)


# ------------------------------------------------------------------ in place
def _through_matmul(V, inplace):
    """The models' use: logits = h @ W (a non-leaf), loss with the default
    mean reduction.  Returns what the matmul's backward was handed."""
    g = torch.Generator(device=DEV).manual_seed(14)
    h = torch.randn(T, 64, device=DEV, generator=g).to(torch.bfloat16).requires_grad_()
    W = (0.4 * torch.randn(64, V, device=DEV, generator=g)).to(torch.bfloat16).requires_grad_()
    tgt = _targets(T, V, 14)
    logits = h @ W
    values = logits.detach().clone()
    seen = {}

    def hook(grad):
        seen["same_storage"] = (grad.untyped_storage().data_ptr() == logits.untyped_storage().data_ptr()
                                and grad.data_ptr() == logits.data_ptr())
        seen["dlogits"] = grad.detach().clone()

    logits.register_hook(hook)
    loss = cross_entropy(logits, tgt, inplace_grad=inplace)
    (loss * 3.0).backward()
    return dict(loss=loss.detach(), h=h.grad, W=W.grad, values=values, tgt=tgt, **seen)


@pytest.mark.parametrize("V", [1000, 1001])
def test_inplace_grad_reuses_the_logits_buffer(V):
    a, b = _through_matmul(V, False), _through_matmul(V, True)
    assert torch.equal(a["values"], b["values"])
    assert not a["same_storage"]
    assert b["same_storage"], "inplace_grad=True must hand the logits' own buffer to the matmul backward"
    assert torch.equal(a["loss"], b["loss"])
    assert torch.equal(a["dlogits"], b["dlogits"])
    assert torch.equal(a["h"], b["h"]) and torch.equal(a["W"], b["W"])
    rloss, rgrad = _ref(a["values"], a["tgt"], lambda l: l * 3.0, reduction="mean")
    _check_loss(f"inplace V={V}", b["loss"], rloss)
    _check_grad_rows(f"inplace V={V}", b["dlogits"], rgrad)


@pytest.mark.parametrize("inplace", [False, True])
@pytest.mark.parametrize("V", [1000, 1001])
def test_non_contiguous_3d_input(V, inplace):
    full = _logits((2, 20, V), 15)
    tg = _targets(40, V, 15).view(2, 20)
    leaf = full.clone().requires_grad_()
    view = leaf[:, :-1]
    assert not view.is_contiguous()
    w = _weights((2, 19), 15)
    loss = cross_entropy(view, tg[:, 1:], reduction="none", inplace_grad=inplace)
    assert loss.shape == (2, 19)
    (loss * w).sum().backward()
    assert torch.equal(leaf.detach(), full), "the caller's logits were overwritten"
    assert bool((leaf.grad[:, -1] == 0).all())
    rloss, rgrad = _ref(full[:, :-1], tg[:, 1:], lambda l: (l * w.double()).sum())
    tag = f"3-D view V={V} inplace={inplace}"
    _check_loss(tag, loss.detach(), rloss)
    _check_grad_rows(tag, leaf.grad[:, :-1], rgrad)


# ------------------------------------------------------------------ masked
def _check_peak_target_row(grad, rgrad, row, g_row):
    """A row whose target is a logit 60 above the rest: the reference gradient
    is about -V e^-60 at the target, which fp32 cannot hold next to 1 (p - 1
    with p = 1 - 1e-23 is 0).  The relative bound has no meaning there; the
    row is held elementwise to one fp32 ulp of 1 times the upstream gradient."""
    err = (grad[row].double() - rgrad[row]).abs().max()
    assert float(err) <= 2.0 ** -23 * abs(float(g_row)), float(err)


@pytest.mark.parametrize("case", ["first_chunk", "every_third", "single_finite", "peaked"])
def test_masked_vocabulary(case):
    V = 4096
    x = _logits((T, V), 16)
    cls = torch.arange(V)
    allowed, masked, loose = None, torch.zeros(T, V, dtype=torch.bool, device=DEV), None
    if case == "first_chunk":      # thread 0 starts on an all -inf chunk and later sees finite ones
        masked[:, :8] = True
        allowed = cls[8:]
    elif case == "every_third":
        masked[:, ::3] = True
        allowed = cls[cls % 3 != 0]
    tgt = _targets(T, V, 16, allowed=allowed)
    if case == "single_finite":    # row 5: one finite logit, which is the target
        masked[5] = True
        masked[5, 1234] = False
        tgt[5] = 1234
    x[masked] = NEG
    if case == "peaked":           # one logit 60 above the rest: not the target (row 5), the target (row 6)
        x[5, 777] = x[5].float().max() + 60
        x[6, 4001] = x[6].float().max() + 60
        tgt[5], tgt[6] = 12, 4001
        loose = [6]
    assert not bool(masked[torch.arange(T, device=DEV)[tgt >= 0], tgt[tgt >= 0]].any())
    w = _weights((T,), 16)
    loss, grad = _hip_run(x, tgt, lambda l: (l * w).sum(), reduction="none")
    rloss, rgrad = _ref(x, tgt, lambda l: (l * w.double()).sum())
    assert bool(torch.isfinite(rloss).all()) and bool(torch.isfinite(rgrad).all())
    assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(grad).all())
    _check_loss(f"masked {case}", loss, rloss)
    _check_grad_rows(f"masked {case}", grad, rgrad, skip_rows=loose)
    assert bool((grad[masked] == 0).all()), "masked classes must get exactly zero gradient"
    if case == "single_finite":
        assert float(loss[5]) == 0.0 and bool((grad[5] == 0).all())
    if case == "peaked":
        _check_peak_target_row(grad, rgrad, 6, w[6])


# ------------------------------------------------------------------ vocab slices
def test_vocab_slice_mode_of_the_c_entry():
    """Two slices of a V = 1000 row through ``dw_xent_fwd`` / ``dw_xent_bwd``
    (``vocab_start`` 0 and 504; smoothing 0 -- in slice mode it would divide
    by the local width).  rowmax / rowsum combine on the host into the global
    lse; the per-slice ``lse_i - x_t`` pieces (x_t = 0 outside the slice) give
    the loss; the backward with the combined lse gives the full gradient."""
    V, cut = 1000, 504
    L = _hip.lib()
    x = _logits((T, V), 17)
    tgt = _targets(T, V, 17)
    tgt[5], tgt[6] = cut - 1, cut  # either side of the cut
    w = _weights((T,), 17)
    rloss, rgrad = _ref(x, tgt, lambda l: (l * w.double()).sum())
    ref_lse = torch.logsumexp(x.double(), dim=-1)
    slices = [(0, x[:, :cut].contiguous()), (cut, x[:, cut:].contiguous())]
    assert slices[1][1].shape[1] == 496
    fwd = []
    for start, xs in slices:
        o = {k: torch.full((T,), float("nan"), device=DEV) for k in ("loss", "lse", "max", "sum")}
        _hip.check(L.dw_xent_fwd(_hip.ptr(xs), _hip.ptr(tgt), _hip.ptr(o["loss"]), _hip.ptr(o["lse"]),
                                 _hip.ptr(o["max"]), _hip.ptr(o["sum"]), T, xs.shape[1], -100, start, 0.0,
                                 _hip.stream()), "xent_fwd")
        assert all(bool(torch.isfinite(v).all()) for v in o.values())
        assert bool((o["loss"][tgt == -100] == 0).all())
        # the slice's own statistics
        assert float((o["max"].double() - xs.double().amax(-1)).abs().max()) == 0.0
        assert float((o["lse"].double() - torch.logsumexp(xs.double(), -1)).abs().max()) <= LOSS_TOL
        fwd.append(o)
    M = torch.maximum(fwd[0]["max"], fwd[1]["max"]).double()
    S = sum(o["sum"].double() * (o["max"].double() - M).exp() for o in fwd)
    lse = M + S.log()
    assert float((lse - ref_lse).abs().max()) <= LOSS_TOL
    valid = tgt != -100
    x_t = sum(o["lse"].double() - o["loss"].double() for o in fwd)  # lse_i - (lse_i - x_t or 0)
    loss = torch.where(valid, lse - x_t, torch.zeros_like(lse))
    _check_loss("vocab slices", loss.float(), rloss)
    lse32 = lse.float()
    parts = []
    for start, xs in slices:
        dx = torch.full_like(xs, float("nan"))
        _hip.check(L.dw_xent_bwd(_hip.ptr(xs), _hip.ptr(tgt), _hip.ptr(lse32), _hip.ptr(w), 1, _hip.ptr(dx), T,
                                 xs.shape[1], -100, start, 0.0, _hip.stream()), "xent_bwd")
        parts.append(dx)
    _check_grad_rows("vocab slices", torch.cat(parts, dim=1), rgrad)
