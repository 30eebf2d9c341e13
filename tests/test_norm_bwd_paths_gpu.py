"""Norm backward (dw_norm_bwd, csrc/kernels/colred.hip): every path of its
dispatch table (docs/norm_backward.md) at the hidden sizes where the path
changes, ragged and multi-step row loops, the scratch contracts and the
entry's argument validation.  Reference: fp32 PyTorch autograd, relative L2
error < 2e-2 as in test_ops_gpu.py / test_norm_fold_gpu.py."""

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL = 2e-2


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dlrover_wuqiong_amd._native import kernels

    kernels(required=True)


def _rel(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def _inputs(R, H, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    x, r, dy, dh = (torch.randn(R, H, generator=g).to(DEV, torch.bfloat16) for _ in range(4))
    w = (1 + 0.1 * torch.randn(H, generator=g)).to(DEV, torch.bfloat16)
    b = (0.1 * torch.randn(H, generator=g)).to(DEV, torch.bfloat16)
    return x, r, dy, dh, w, b


def _ref_norm(h, w, b, rms):
    if rms:
        return h * torch.rsqrt(h.pow(2).mean(-1, keepdim=True) + 1e-6) * w
    return F.layer_norm(h, (h.shape[-1],), w, b, 1e-5)


def _run(x, r, dy, dh, w, b, rms, add):
    """(dx, dgamma, dbeta or None) of the HIP path; ``add``: the fused
    add+norm with a gradient on the residual output."""
    from dlrover_wuqiong_amd.ops.norm import add_layer_norm, add_rms_norm, layer_norm, rms_norm

    x, w, b = x.clone().requires_grad_(), w.clone().requires_grad_(), b.clone().requires_grad_()
    if add:
        y, h = add_rms_norm(x, r, w, 1e-6) if rms else add_layer_norm(x, r, w, b, 1e-5)
        torch.autograd.backward([y, h], [dy, dh])
    else:
        y = rms_norm(x, w, 1e-6) if rms else layer_norm(x, w, b, 1e-5)
        y.backward(dy)
    return x.grad, w.grad, None if rms else b.grad


def _ref(x, r, dy, dh, w, b, rms, add):
    xf, wf, bf = (t.float().requires_grad_() for t in (x, w, b))
    if add:
        hf = xf + r.float()
        torch.autograd.backward([_ref_norm(hf, wf, bf, rms), hf], [dy.float(), dh.float()])
    else:
        _ref_norm(xf, wf, bf, rms).backward(dy.float())
    return xf.grad, wf.grad, None if rms else bf.grad


def _check(got, ref):
    for name, a, e in zip(("dx", "dgamma", "dbeta"), got, ref):
        if e is not None:
            err = _rel(a, e)
            print(name, err)
            assert err < TOL, (name, err)


# 1024 / 1032: last one-wave size, first wave-pair size; 2040 / 2048: last pair
# size (255 vectors: a ragged last lane group), first wave-quad size; 4096 /
# 4104: last quad size, first two-pass size.  37 rows: several workgroups, the
# last one ragged, on every path.
@pytest.mark.parametrize("H", [1024, 1032, 2040, 2048, 4096, 4104])
@pytest.mark.parametrize("rms", [False, True])
def test_every_boundary_of_the_dispatch_table(H, rms):
    t = _inputs(37, H)
    for add in (False, True):
        _check(_run(*t, rms, add), _ref(*t, rms, add))


# R = 3: fewer rows than one workgroup's row groups.  1027 rows at H = 1600:
# 256 workgroups x 4 wave pairs, one workgroup takes a second step; 515 at
# 4096: the same for 2 wave quads; 2051 at 512: 512 workgroups x 4 waves.
@pytest.mark.parametrize("R,H", [(3, 1600), (3, 4096), (1027, 1600), (515, 4096), (2051, 512)])
@pytest.mark.parametrize("rms", [False, True])
@pytest.mark.parametrize("det", [False, True])
def test_ragged_and_multi_step_row_loops(R, H, rms, det, monkeypatch):
    if det:
        monkeypatch.setenv("DWAMD_DETERMINISTIC", "1")
    t = _inputs(R, H, seed=1)
    got = _run(*t, rms, True)
    _check(got, _ref(*t, rms, True))
    if det:
        for a, b in zip(got, _run(*t, rms, True)):
            assert b is None or torch.equal(a, b)


def _entry(R, H, rms=False, dsum=False, det=False, part_short=0, null_dgamma=False, fill=None):
    """One direct dw_norm_bwd call; returns (status, outputs dict)."""
    from dlrover_wuqiong_amd.ops import _hip

    x, _, dy, dres, w, _ = _inputs(R, H, seed=2)
    xf = x.float()
    mean = torch.zeros(R, device=DEV) if rms else xf.mean(-1).contiguous()
    rstd = ((xf.pow(2).mean(-1) if rms else xf.var(-1, unbiased=False)) + 1e-5).rsqrt().contiguous()
    out = {"dx": torch.empty_like(x), "dgamma": torch.empty(H, device=DEV), "dbeta": torch.empty(H, device=DEV),
           "dsum": torch.empty(H, device=DEV)}
    if fill is not None:
        for v in out.values():
            v.fill_(fill)
    L = _hip.lib()
    need = L.dw_norm_bwd_part_floats(R, H, int(dsum))
    part = torch.empty(max(need, 1), device=DEV)
    ws = _hip.zeroed_workspace(3 * H + max((H + 511) // 512, (3 * H + 255) // 256), DEV)
    st = L.dw_norm_bwd(_hip.ptr(dy), _hip.ptr(x), _hip.ptr(w), _hip.ptr(mean), _hip.ptr(rstd), _hip.ptr(dres),
                       _hip.ptr(out["dx"]), _hip.ptr(None if null_dgamma else out["dgamma"]),
                       _hip.ptr(None if rms else out["dbeta"]), _hip.ptr(ws), _hip.ptr(part), need - part_short, R, H,
                       int(rms), 1, 2, _hip.ptr(out["dsum"] if dsum else None), _hip.stream(),
                       _hip.det_scratch(R, H, 2, DEV) if det else None)
    torch.cuda.synchronize()
    return st, out


def _ws_words(H):
    return 3 * H + max((H + 511) // 512, (3 * H + 255) // 256)


@pytest.mark.parametrize("H", [512, 1600, 4096, 4104])
@pytest.mark.parametrize("det", [False, True])
def test_zeroed_workspace_left_zero(H, det, monkeypatch):
    """``ws`` is zero on entry and on exit on each of the four paths, with the
    atomic and with the ordered combine, with and without the dx column sums."""
    from dlrover_wuqiong_amd.ops import _hip

    if det:
        monkeypatch.setenv("DWAMD_DETERMINISTIC", "1")
    n = _ws_words(H)
    t = _inputs(130, H, seed=3)
    for rms in (False, True):
        _run(*t, rms, True)
        torch.cuda.synchronize()
        assert int((_hip.zeroed_workspace(n, DEV)[:n] != 0).sum()) == 0
    if H < 2048:
        st, _ = _entry(130, H, dsum=True, det=det)
        assert st == 0
        assert int((_hip.zeroed_workspace(n, DEV)[:n] != 0).sum()) == 0


def test_part_floats():
    from dlrover_wuqiong_amd.ops import _hip

    pf = _hip.lib().dw_norm_bwd_part_floats
    for R in (3, 777, 8192):
        assert pf(R, 4104, 0) == 0 and pf(R, 8192, 0) == 0
        for H in (8, 512, 1024, 1032, 1600, 2040, 2048, 4096):
            assert pf(R, H, 0) > 0
        for H in (512, 1600):
            assert 2 * pf(R, H, 1) == 3 * pf(R, H, 0)


@pytest.mark.parametrize("case", ["H=1604", "H=8200", "null dgamma", "dsum at H=2048", "part one float short"])
def test_entry_rejects_without_launching(case):
    """A non-zero status and untouched outputs: nothing was launched."""
    kw = {"H=1604": dict(H=1604), "H=8200": dict(H=8200), "null dgamma": dict(H=512, null_dgamma=True),
          "dsum at H=2048": dict(H=2048, dsum=True), "part one float short": dict(H=1600, part_short=1)}[case]
    st, out = _entry(64, fill=-7.0, **kw)
    assert st != 0
    for name, v in out.items():
        assert bool((v == -7.0).all()), name


def test_entry_accepts_the_exact_part_size():
    st, out = _entry(64, 1600, dsum=True, fill=-7.0)
    assert st == 0
    assert not bool((out["dx"] == -7.0).all()) and not bool((out["dsum"] == -7.0).any())


@pytest.mark.parametrize("H", [512, 1600, 4096, 4104])
def test_layer_norm_without_bias(H):
    """``LayerNorm(H, bias=False)``: a null dbeta on the LayerNorm kernels."""
    from dlrover_wuqiong_amd.ops.norm import LayerNorm

    x, _, dy, _, w, _ = _inputs(130, H, seed=4)
    m = LayerNorm(H, bias=False, device=DEV, dtype=torch.bfloat16)
    with torch.no_grad():
        m.weight.copy_(w)
    xi = x.clone().requires_grad_()
    y = m(xi)
    y.backward(dy)
    xf, wf = x.float().requires_grad_(), w.float().requires_grad_()
    yf = F.layer_norm(xf, (H,), wf, torch.zeros(H, device=DEV), 1e-5)
    yf.backward(dy.float())
    assert _rel(y, yf) < 1e-2
    _check((xi.grad, m.weight.grad), (xf.grad, wf.grad))
