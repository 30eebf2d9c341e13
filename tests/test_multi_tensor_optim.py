"""Multi-tensor fused AdamW / AGD (``optimizers/multi_tensor.py``,
``csrc/kernels/optim_multi.hip``): CPU reference math vs torch.optim / ATorch
AGD, state-dict layout, auto_accelerate wiring incl. FSDP2 (gloo, 2 ranks)
with a flash-checkpoint round trip; GPU kernel vs the fp32 reference."""

import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import free_port, gpu_available
from dlrover_wuqiong_amd.optimizers.agd import AGD
from dlrover_wuqiong_amd.optimizers.multi_tensor import MultiTensorAdamW, MultiTensorAGD, fused_equivalent


def _params(dtype=torch.float32, device="cpu", seed=0):
    g = torch.Generator().manual_seed(seed)
    shapes = [(37, 19), (1000,), (3, 5, 7), (64, 64), (1,)]
    return [torch.randn(s, generator=g).to(device=device, dtype=dtype).requires_grad_() for s in shapes]


def _grads(ps, step):
    g = torch.Generator().manual_seed(100 + step)
    return [torch.randn(p.shape, generator=g).to(p.device) for p in ps]


def _groups(ps, **extra):
    return [{"params": ps[:3]}, {"params": ps[3:], "weight_decay": 0.0, **extra}]


@pytest.mark.parametrize("adamw", [True, False])
def test_adam_matches_torch(adamw):
    ps, ref = _params(), _params()
    o = MultiTensorAdamW(_groups(ps), lr=1e-2, weight_decay=0.1, adamw=adamw)
    cls = torch.optim.AdamW if adamw else torch.optim.Adam
    r = cls(_groups(ref), lr=1e-2, weight_decay=0.1)
    for s in range(6):
        for a, b, g in zip(ps, ref, _grads(ps, s)):
            a.grad, b.grad = g.clone(), g.clone()
        o.step()
        r.step()
    for a, b in zip(ps, ref):
        torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-6)


def test_agd_matches_reference():
    ps, ref = _params(), _params()
    o = MultiTensorAGD(_groups(ps, clip=0.5), lr=1e-2, weight_decay=0.05, delta=1e-5)
    r = AGD(_groups(ref, clip=0.5), lr=1e-2, weight_decay=0.05, delta=1e-5)
    for s in range(6):
        for a, b, g in zip(ps, ref, _grads(ps, s)):
            a.grad, b.grad = g.clone(), g.clone()
        o.step()
        r.step()
    for a, b in zip(ps, ref):
        torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("kind", ["adamw", "adam_l2", "agd"])
def test_shared_cpu_update_matches_reference(kind, masked):
    """``_ref_math.adam_update_`` / ``agd_update_`` -- the one CPU update every
    fused class runs -- with ``decay=None`` and with an all-true mask, against
    torch.optim.AdamW / Adam and the AGD reference: 3 tensors, 4 steps."""
    from dlrover_wuqiong_amd.optimizers._ref_math import adam_update_, agd_update_

    ws, ref = _params()[:3], _params()[:3]
    lr, b1, b2, wd = 1e-2, 0.9, 0.999, 0.1
    if kind == "agd":
        r = AGD(ref, lr=lr, betas=(b1, b2), delta=1e-5, weight_decay=wd, clip=0.5)
    else:
        r = (torch.optim.AdamW if kind == "adamw" else torch.optim.Adam)(ref, lr=lr, betas=(b1, b2), eps=1e-8,
                                                                        weight_decay=wd)
    ms, vs = [torch.zeros_like(w) for w in ws], [torch.zeros_like(w) for w in ws]
    for t in range(1, 5):
        bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
        for w, b, g, m, v in zip(ws, ref, _grads(ws, t), ms, vs):
            b.grad = g.clone()
            decay = torch.ones_like(w, dtype=torch.bool) if masked else None
            with torch.no_grad():
                if kind == "agd":
                    agd_update_(w, g, m, v, lr=lr, b1=b1, b2=b2, delta=1e-5, wd=wd, bc1=bc1, bc2=bc2,
                                bc1_prev=(1.0 - b1 ** (t - 1)) if t > 1 else 0.0, clip=0.5, decay=decay)
                else:
                    adam_update_(w, g, m, v, lr=lr, b1=b1, b2=b2, eps=1e-8, wd=wd, bc1=bc1, bc2=bc2,
                                 adamw=kind == "adamw", decay=decay)
        r.step()
    for w, b in zip(ws, ref):
        torch.testing.assert_close(w, b, rtol=1e-5, atol=1e-6)


def test_bf16_params_keep_fp32_master():
    ps = _params(torch.bfloat16)
    ref = [p.detach().float().clone().requires_grad_() for p in ps]
    o = MultiTensorAdamW(ps, lr=1e-3, weight_decay=0.1)
    r = torch.optim.AdamW(ref, lr=1e-3, weight_decay=0.1)
    assert all("master_param" in o.state[p] for p in ps)
    for s in range(5):
        for a, b, g in zip(ps, ref, _grads(ps, s)):
            a.grad, b.grad = g.to(torch.bfloat16), g.to(torch.bfloat16).float()
        o.step()
        r.step()
    for a, b in zip(ps, ref):
        torch.testing.assert_close(o.state[a]["master_param"], b.detach(), rtol=1e-5, atol=1e-6)
        assert torch.equal(a.detach(), b.detach().to(torch.bfloat16))


def test_grad_clipping_matches_clip_grad_norm():
    ps, ref = _params(), _params()
    o = MultiTensorAdamW(ps, lr=1e-2, max_grad_norm=0.5)
    r = torch.optim.AdamW(ref, lr=1e-2)
    for s in range(4):
        for a, b, g in zip(ps, ref, _grads(ps, s)):
            a.grad, b.grad = 3 * g, 3 * g
        o.step()
        nrm = torch.nn.utils.clip_grad_norm_(ref, 0.5)
        r.step()
        assert abs(float(o.last_grad_norm) - float(nrm)) < 1e-3 * float(nrm)
    for a, b in zip(ps, ref):
        torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-6)


def test_state_is_flat_views_and_load_keeps_them():
    ps = _params()
    o = MultiTensorAdamW(ps, lr=1e-2)
    for a, g in zip(ps, _grads(ps, 0)):
        a.grad = g
    o.step()
    flat = o.flat_state_buffers()[torch.device("cpu")]
    base = flat["exp_avg"].data_ptr()
    ptrs = [o.state[p]["exp_avg"].data_ptr() for p in ps]
    assert all(base <= x < base + flat["exp_avg"].numel() * 4 for x in ptrs)
    sd = o.state_dict()
    saved = {i: {k: (v.clone() if torch.is_tensor(v) else v) for k, v in s.items()} for i, s in sd["state"].items()}
    for a, g in zip(ps, _grads(ps, 1)):
        a.grad = g
    o.step()
    o.load_state_dict({"state": saved, "param_groups": sd["param_groups"]})
    assert [o.state[p]["exp_avg"].data_ptr() for p in ps] == ptrs
    assert o.step_count == 1
    for i, p in enumerate(ps):
        assert torch.equal(o.state[p]["exp_avg"], saved[i]["exp_avg"])


def test_fused_equivalent_mapping():
    assert fused_equivalent(torch.optim.AdamW, {})[0] is MultiTensorAdamW
    cls, args = fused_equivalent(torch.optim.Adam, {"lr": 1.0})
    assert cls is MultiTensorAdamW and args["adamw"] is False and args["weight_decay"] == 0.0
    assert fused_equivalent(torch.optim.AdamW, {"amsgrad": True})[0] is None
    assert fused_equivalent(AGD, {"clip": 1.0})[0] is MultiTensorAGD
    assert fused_equivalent(AGD, {"win": True})[0] is None
    assert fused_equivalent(torch.optim.SGD, {})[0] is None


def test_auto_accelerate_uses_fused_optimizer():
    from dlrover_wuqiong_amd.atorch.auto_accelerate import auto_accelerate

    model = torch.nn.Sequential(torch.nn.Linear(8, 16), torch.nn.ReLU(), torch.nn.Linear(16, 4))
    ok, res, _ = auto_accelerate(model, torch.optim.AdamW, optim_args={"lr": 1e-3}, load_strategy=["half"])
    assert ok and isinstance(res.optim, MultiTensorAdamW)
    assert all("master_param" in s for s in res.optim.state.values())
    ok, res, _ = auto_accelerate(model, torch.optim.AdamW, optim_args={"lr": 1e-3}, load_strategy=[],
                                 fused_optimizer=False)
    assert type(res.optim) is torch.optim.AdamW


# ----------------------------------------------------------- FSDP2 (gloo)
def _fsdp_worker(rank, world, port, root, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), LOCAL_WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from torch.distributed.fsdp import fully_shard

        from dlrover_wuqiong_amd.flash_checkpoint.checkpointer import StorageType
        from dlrover_wuqiong_amd.flash_checkpoint.fsdp import FsdpShardCheckpointer

        torch.manual_seed(0)
        model = torch.nn.Sequential(torch.nn.Linear(8, 16), torch.nn.ReLU(), torch.nn.Linear(16, 5))
        ref = torch.nn.Sequential(torch.nn.Linear(8, 16), torch.nn.ReLU(), torch.nn.Linear(16, 5))
        ref.load_state_dict(model.state_dict())
        for m in model:
            if isinstance(m, torch.nn.Linear):
                fully_shard(m)
        fully_shard(model)
        opt = MultiTensorAdamW(model.parameters(), lr=1e-2, weight_decay=0.1, max_grad_norm=1.0)
        ropt = torch.optim.AdamW(ref.parameters(), lr=1e-2, weight_decay=0.1)

        def train(seed):
            g = torch.Generator().manual_seed(seed)
            x = torch.randn(4, 8, generator=g)
            model(x).pow(2).sum().backward()
            opt.step()
            opt.zero_grad()
            # the replicated reference sees the mean over ranks of the same batch
            ref(x).pow(2).sum().backward()
            torch.nn.utils.clip_grad_norm_(ref.parameters(), 1.0)
            ropt.step()
            ropt.zero_grad()

        for s in range(3):
            train(s)
        full = {k: v.full_tensor() for k, v in model.state_dict().items()}
        ok = all(torch.allclose(full[k], v, rtol=1e-5, atol=1e-6) for k, v in ref.state_dict().items())
        ck = FsdpShardCheckpointer(root)
        assert ck.save_checkpoint(3, model, opt, storage_type=StorageType.MEMORY)
        ck.wait_latest_checkpoint()
        want = {k: v.to_local().clone() for k, v in model.state_dict().items()}
        want_m = [opt.state[p]["exp_avg"].to_local().clone() for p in model.parameters()]
        train(7)
        ck.load_checkpoint(model, opt)
        ok = ok and all(torch.equal(v.to_local(), want[k]) for k, v in model.state_dict().items())
        ok = ok and all(torch.equal(opt.state[p]["exp_avg"].to_local(), w)
                        for p, w in zip(model.parameters(), want_m))
        ok = ok and opt.step_count == 3
        ck.close()
        q.put((rank, bool(ok)))
    except Exception as e:  # pragma: no cover - reported to the parent
        import traceback

        q.put((rank, traceback.format_exc() + repr(e)))
    finally:
        dist.destroy_process_group()


def test_fsdp2_multi_tensor_matches_replicated_and_flash_ckpt(tmp_path):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=_fsdp_worker, args=(r, 2, port, str(tmp_path), q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=240) for _ in procs)
    for p in procs:
        p.join(timeout=60)
    assert res == {0: True, 1: True}, res


# ----------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("pdtype,gdtype,agd", [(torch.float32, torch.float32, False),
                                               (torch.bfloat16, torch.bfloat16, False),
                                               (torch.bfloat16, torch.float32, False),
                                               (torch.bfloat16, torch.bfloat16, True)])
def test_gpu_kernel_matches_cpu_reference(pdtype, gdtype, agd):
    assert gpu_available()
    dev = torch.device("cuda:0")
    # include a misaligned view (scalar path) and a multi-chunk tensor
    big = torch.randn(3 * 16384 + 77, generator=torch.Generator().manual_seed(3))
    shapes = [(37, 19), (1000,), (64, 64), (1,)]
    g0 = torch.Generator().manual_seed(5)
    cpu = [torch.randn(s, generator=g0) for s in shapes] + [big]
    store = torch.zeros(cpu[1].numel() + 1, dtype=pdtype, device=dev)
    gp = []
    for i, c in enumerate(cpu):
        if i == 1:  # element offset 1: not 16-byte aligned
            v = store[1:].view(c.shape)
            v.data.copy_(c.to(pdtype))
            gp.append(torch.nn.Parameter(v))
        else:
            gp.append(torch.nn.Parameter(c.to(device=dev, dtype=pdtype)))
    rp = [torch.nn.Parameter(p.detach().float().cpu()) for p in gp]
    kw = dict(lr=1e-2, weight_decay=0.1, max_grad_norm=2.0)
    groups = lambda ps: [{"params": ps[:3]}, {"params": ps[3:], "weight_decay": 0.0}]  # noqa: E731
    if agd:
        o, r = MultiTensorAGD(groups(gp), clip=1.0, **kw), MultiTensorAGD(groups(rp), clip=1.0, **kw)
    else:
        o, r = MultiTensorAdamW(groups(gp), **kw), MultiTensorAdamW(groups(rp), **kw)
    for s in range(5):
        for a, b, g in zip(gp, rp, _grads(rp, s)):
            gq = g.to(gdtype)
            if gdtype != pdtype and hasattr(a, "grad_dtype"):
                a.grad_dtype = None  # fp32 grads on bf16 params (e.g. FSDP2 reduce_dtype=fp32)
            a.grad = gq.to(dev)
            b.grad = gq.float()
        o.step()
        r.step()
    torch.cuda.synchronize()
    for a, b in zip(gp, rp):
        w = o.state[a]["master_param"] if "master_param" in o.state[a] else a
        wr = r.state[b]["master_param"] if "master_param" in r.state[b] else b
        torch.testing.assert_close(w.detach().float().cpu(), wr.detach(), rtol=2e-5, atol=2e-5)
        torch.testing.assert_close(o.state[a]["exp_avg_sq"].cpu(), r.state[b]["exp_avg_sq"], rtol=1e-4, atol=1e-7)
    assert abs(float(o.last_grad_norm) - float(r.last_grad_norm)) < 1e-3 * float(r.last_grad_norm)


@pytest.mark.gpu
def test_gpu_multi_tensor_vs_torch_adamw_fp32():
    assert gpu_available()
    dev = torch.device("cuda:0")
    ps = _params(device=dev)
    ref = [p.detach().float().cpu().clone().requires_grad_() for p in ps]
    o = MultiTensorAdamW(ps, lr=3e-3, betas=(0.9, 0.95), weight_decay=0.1)
    r = torch.optim.AdamW(ref, lr=3e-3, betas=(0.9, 0.95), weight_decay=0.1)
    for s in range(8):
        for a, b, g in zip(ps, ref, _grads(ref, s)):
            a.grad, b.grad = g.to(dev), g.clone()
        o.step()
        r.step()
    for a, b in zip(ps, ref):
        torch.testing.assert_close(a.detach().cpu(), b.detach(), rtol=1e-5, atol=1e-5)


# ------------------------------- multi-tensor == flat kernels, bit for bit
_DTYPES = [(torch.float32, torch.float32), (torch.bfloat16, torch.bfloat16), (torch.bfloat16, torch.float32),
           (torch.float32, torch.bfloat16)]


def _mt_equals_flat(agd, pdtype, gdtype, wd, adamw=1, clip=0.0):
    """Two consecutive steps of ``dw_mt_adam`` (one launch over every tensor)
    and of ``dw_adam_flat`` / ``dw_agd_flat`` (one launch per tensor, on its
    own aligned buffers, every element decaying) from the same seeded values:
    parameters, masters and both moments must be the same bits.  Sizes: the
    scalar tail (1, 7), one vector (8), a 64-block, a tensor whose parameter
    sits 1 element off 16-byte alignment (200: the scalar path) and a chunk
    crossing; two param groups with their own lr; a device gradient scale."""
    import ctypes

    import numpy as np

    from dlrover_wuqiong_amd.ops import _hip
    from dlrover_wuqiong_amd.optimizers import multi_tensor as mt

    assert gpu_available()
    dev = torch.device("cuda:0")
    L = _hip.lib()
    chunk = int(L.dw_mt_chunk())
    sizes = [1, 7, 8, 64, 200, chunk + 9]
    gen = torch.Generator().manual_seed(11)
    b1, b2, eps, lrs = 0.9, 0.95, 1e-6, (1e-2, 3e-3)
    gscale = torch.tensor([0.37], device=dev)
    multi, flat = [], []
    for n in sizes:
        w0 = torch.randn(n, generator=gen).to(dev)
        off = 1 if n == 200 else 0
        p = torch.zeros(n + off, dtype=pdtype, device=dev)[off:]
        p.copy_(w0)
        t = {"p": p, "master": w0.clone() if pdtype != torch.float32 else None,
             "m": torch.zeros(n, device=dev), "v": torch.zeros(n, device=dev)}
        multi.append(t)
        flat.append({k: None if x is None else x.clone() for k, x in t.items()})
    assert multi[4]["p"].data_ptr() % 16 != 0 and flat[4]["p"].data_ptr() % 16 == 0
    for step in (1, 2):
        bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
        bc1_prev = 1.0 - b1 ** (step - 1) if step > 1 else 0.0
        grads = [torch.randn(n, generator=gen).to(gdtype).to(dev) for n in sizes]
        desc = np.zeros(len(sizes), dtype=mt._DESC)
        chunks = []
        for ti, (t, g) in enumerate(zip(multi, grads)):
            ptrs = [x.data_ptr() for x in (t["p"], g, t["m"], t["v"], t["master"]) if x is not None]
            flags = (pdtype == torch.bfloat16) | 2 * (gdtype == torch.bfloat16) | 4 * all(x % 16 == 0 for x in ptrs)
            desc[ti] = (t["p"].data_ptr(), g.data_ptr(), 0 if t["master"] is None else t["master"].data_ptr(),
                        t["m"].data_ptr(), t["v"].data_ptr(), sizes[ti], flags, ti % 2, 1.0, 0)
            chunks += [(ti, c) for c in range((sizes[ti] + chunk - 1) // chunk)]
        h = {k: np.zeros(mt.MAX_GROUPS, dtype=np.float32) for k in mt._HYPER_FIELDS}
        for gi, lr in enumerate(lrs):
            for k, x in (("lr", lr), ("wd", wd), ("b1", b1), ("b2", b2), ("eps", eps), ("bc1", bc1), ("bc2", bc2),
                         ("bc1_prev", bc1_prev), ("clip", clip)):
                h[k][gi] = x
        raw = np.concatenate([h[k] for k in mt._HYPER_FIELDS] + [np.array([adamw], dtype=np.int32).view(np.float32)])
        assert raw.nbytes == int(L.dw_mt_hyper_size())
        d_desc = torch.from_numpy(desc.view(np.uint8).copy()).to(dev)
        d_chunks = torch.tensor(chunks, dtype=torch.int32, device=dev)
        _hip.check(L.dw_mt_adam(_hip.ptr(d_desc), _hip.ptr(d_chunks), len(chunks), _hip.ptr(gscale),
                                ctypes.c_void_p(raw.ctypes.data), int(agd), _hip.stream()), "mt_step")
        for ti, (t, g) in enumerate(zip(flat, grads)):
            head = (_hip.ptr(t["p"]), _hip.dtype_code(t["p"]), _hip.ptr(t["master"]), _hip.ptr(g), _hip.dtype_code(g),
                    _hip.ptr(t["m"]), _hip.ptr(t["v"]), _hip.ptr(gscale), sizes[ti], sizes[ti], lrs[ti % 2], b1, b2,
                    eps, wd, bc1)
            if agd:
                _hip.check(L.dw_agd_flat(*head, bc1_prev, bc2, clip, None, _hip.stream()), "agd")
            else:
                _hip.check(L.dw_adam_flat(*head, bc2, adamw, None, _hip.stream()), "adam")
        torch.cuda.synchronize()
        for ti, (a, b) in enumerate(zip(multi, flat)):
            for k in ("p", "master", "m", "v"):
                if a[k] is not None:
                    assert torch.equal(a[k], b[k]), (step, sizes[ti], k, (a[k].float() - b[k].float()).abs().max())
        assert float(multi[-1]["v"].min()) > 0  # the update ran


@pytest.mark.gpu
@pytest.mark.parametrize("wd", [0.0, 0.1])
@pytest.mark.parametrize("adamw", [1, 0])
@pytest.mark.parametrize("pdtype,gdtype", _DTYPES)
def test_gpu_multi_tensor_adam_equals_flat_bit_for_bit(pdtype, gdtype, adamw, wd):
    _mt_equals_flat(False, pdtype, gdtype, wd, adamw=adamw)


@pytest.mark.gpu
@pytest.mark.parametrize("clip", [0.0, 0.5])
@pytest.mark.parametrize("pdtype,gdtype", _DTYPES)
def test_gpu_multi_tensor_agd_equals_flat_bit_for_bit(pdtype, gdtype, clip):
    _mt_equals_flat(True, pdtype, gdtype, 0.1, clip=clip)
