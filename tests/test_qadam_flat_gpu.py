"""GPU: the flat AdamW kernel with 8-/4-bit block-quantized moments
(optim_qflat.hip, dw_qadam_flat) against a torch fp32 reference of the same
update (decode -> update -> encode with the optimizers/low_bit.py codec),
against dw_adam_flat on the decoded state, and FusedQAdamW end to end (CPU
path, flash checkpoint, auto_accelerate)."""

import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
HP = dict(lr=1e-2, b1=0.9, b2=0.95, eps=1e-8, wd=0.1, bc1=1 - 0.9 ** 3, bc2=1 - 0.95 ** 3)
GUARD = 256  # elements after the updated range that must stay untouched


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _npad(n):
    return (n + 127) // 128 * 128


def _unpack(codes, bits):
    from dlrover_wuqiong_amd.optimizers.low_bit import _unpack4

    return _unpack4(codes) if bits == 4 else codes


def _pack(codes, bits):
    from dlrover_wuqiong_amd.optimizers.low_bit import _pack4

    return _pack4(codes.reshape(-1)) if bits == 4 else codes.reshape(-1).contiguous()


def _decode(c, bits, a, b):
    """fp32 (m, v) of the flat elements [a, b) (multiples of 128) with the
    torch codec, run on the CPU: there ``scale / 127.0`` is the division the
    kernels do.  On the GPU torch turns a division by a Python scalar into a
    multiplication by its reciprocal, which decodes 3.5 % of the 8-bit first
    moments one ulp off (measured: 37352 of 1048576) -- enough to move 0.1 %
    of the updated masters by an ulp, where the CPU decode moves none."""
    from dlrover_wuqiong_amd.optimizers.low_bit import dequant_m, dequant_v

    G = (b - a) // 128
    ms, vs = c["ms"][a // 128:b // 128].cpu(), c["vs"][a // 128:b // 128].cpu()
    m = dequant_m(_unpack(c["mq"], bits)[a:b].cpu().view(G, 128), ms, bits).reshape(-1)
    v = dequant_v(_unpack(c["vq"], bits)[a:b].cpu().view(G, 128), vs, bits).reshape(-1)
    return m.to(DEV), v.to(DEV)


def _inputs(bits, n, lo, pdt=torch.bfloat16, gdt=torch.bfloat16, master=True, fresh=False, zero_group=None, seed=0):
    """A realistic state over lo + npad(n) + GUARD elements: moments encoded
    from randn * 0.1 / rand * 0.1 (also in the padding of the last group and
    outside the range: the kernel must ignore the former and keep the latter)."""
    from dlrover_wuqiong_amd.optimizers.low_bit import quant_m, quant_v

    g = torch.Generator(device=DEV).manual_seed(seed)
    total = lo + _npad(n) + GUARD
    w = torch.randn(total, device=DEV, generator=g)
    c = {"param": w.to(pdt), "master": w.clone() if master else None,
         "grad": torch.randn(total, device=DEV, generator=g).to(gdt),
         "mask": (torch.rand(total // 64, device=DEV, generator=g) > 0.3).to(torch.uint8),
         "gs": torch.full((1,), 0.5, device=DEV)}
    if zero_group is not None:
        c["grad"][lo + zero_group * 128: lo + (zero_group + 1) * 128] = 0
    m0 = torch.randn(total, device=DEV, generator=g) * 0.1
    v0 = torch.rand(total, device=DEV, generator=g) * 0.1
    if fresh:
        m0.zero_()
        v0.zero_()
    mc, c["ms"] = quant_m(m0.view(-1, 128), bits)
    vc, c["vs"] = quant_v(v0.view(-1, 128), bits)
    c["mq"], c["vq"] = _pack(mc, bits), _pack(vc, bits)
    return c


def _clone(c):
    return {k: (v.clone() if torch.is_tensor(v) else v) for k, v in c.items()}


def _code(t):
    return 1 if t.dtype == torch.bfloat16 else 0


def _launch(c, bits, n, lo=0, adamw=1, gscale=True, n_decay=None, hp=HP):
    """dw_qadam_flat over [lo, lo + n): every pointer offset as the issue of a sub-range is."""
    from dlrover_wuqiong_amd.ops import _hip

    cb = lo if bits == 8 else lo // 2
    ms = c["master"]
    return _hip.lib().dw_qadam_flat(
        _hip.ptr(c["param"][lo:]), _code(c["param"]), _hip.ptr(None if ms is None else ms[lo:]),
        _hip.ptr(c["grad"][lo:]), _code(c["grad"]), _hip.ptr(c["mq"][cb:]), _hip.ptr(c["vq"][cb:]),
        _hip.ptr(c["ms"][lo // 128:]), _hip.ptr(c["vs"][lo // 128:]), _hip.ptr(c["gs"] if gscale else None), n,
        0 if n_decay is None else n_decay, hp["lr"], hp["b1"], hp["b2"], hp["eps"], hp["wd"], hp["bc1"], hp["bc2"],
        adamw, _hip.ptr(c["mask"][lo // 64:] if n_decay is None else None), bits, _hip.stream())


def _reference(c, bits, n, lo=0, adamw=1, gscale=True, n_decay=None, hp=HP):
    """torch fp32 on the GPU: decode, update, encode.  Returns (master [n],
    m codes / v codes (unpacked) and scales of the npad(n) elements)."""
    from dlrover_wuqiong_amd.optimizers.low_bit import quant_m, quant_v

    npad = _npad(n)
    m, v = _decode(c, bits, lo, lo + npad)
    g = c["grad"][lo:lo + n].float() * (0.5 if gscale else 1.0)
    w = (c["master"] if c["master"] is not None else c["param"])[lo:lo + n].float().clone()
    if n_decay is None:
        decay = c["mask"][lo // 64:].repeat_interleave(64)[:n].bool()
    else:
        decay = torch.arange(n, device=DEV) < n_decay
    if not adamw:
        g = torch.where(decay, g + hp["wd"] * w, g)
    # 1 - beta in fp32, as the kernels compute it (1.f - 0.9f is 2.4e-7 above float(1 - 0.9))
    b1, b2 = (torch.tensor(hp[k], dtype=torch.float32, device=DEV) for k in ("b1", "b2"))
    m[:n] = b1 * m[:n] + (1 - b1) * g
    v[:n] = b2 * v[:n] + (1 - b2) * g * g
    m[n:] = 0
    v[n:] = 0
    if adamw:
        w = torch.where(decay, w - hp["lr"] * hp["wd"] * w, w)
    w = w - (hp["lr"] / hp["bc1"]) * m[:n] / (v[:n].sqrt() / hp["bc2"] ** 0.5 + hp["eps"])
    mc, ms = quant_m(m.view(-1, 128), bits)
    vc, vs = quant_v(v.view(-1, 128), bits)
    return w, mc.reshape(-1), vc.reshape(-1), ms, vs


def _m_level(codes, bits):
    """Position of a first-moment code in the ordered list of its levels."""
    c = codes.to(torch.int32)
    if bits == 8:
        return torch.where(c > 127, c - 256, c)
    return torch.where(c >= 8, -(c - 8), c)


def _check(c, before, ref, bits, n, lo=0):
    """The issue's criteria for one kernel step of [lo, lo + n)."""
    torch.cuda.synchronize()
    w, mc, vc, ms, vs = ref
    npad = _npad(n)
    hi = lo + npad
    wk = (c["master"] if c["master"] is not None else c["param"])[lo:lo + n]
    assert bool(torch.isfinite(wk).all())
    torch.testing.assert_close(wk.float(), w, rtol=1e-5, atol=1e-5)
    if c["master"] is not None:
        assert torch.equal(c["param"][lo:lo + n], c["master"][lo:lo + n].to(c["param"].dtype))
    gm, gv = c["ms"][lo // 128:hi // 128], c["vs"][lo // 128:hi // 128]
    assert bool(torch.isfinite(gm).all()) and bool(torch.isfinite(gv).all())
    torch.testing.assert_close(gm, ms, rtol=1e-6, atol=0)
    torch.testing.assert_close(gv, vs, rtol=1e-6, atol=0)
    km, kv = _unpack(c["mq"], bits)[lo:hi], _unpack(c["vq"], bits)[lo:hi]
    dm = (_m_level(km, bits) - _m_level(mc, bits)).abs()
    dv = (kv.to(torch.int32) - vc.to(torch.int32)).abs()
    nbad = int((dm > 0).sum()), int((dv > 0).sum())
    print(f"bits={bits} n={n} lo={lo}: codes off by one level: m {nbad[0]}, v {nbad[1]} of {n}")
    assert int(dm.max()) <= 1 and int(dv.max()) <= 1
    assert nbad[0] <= 0.001 * n and nbad[1] <= 0.001 * n
    # padding of the last group: codes exactly 0
    assert int(km[n:].count_nonzero()) == 0 and int(kv[n:].count_nonzero()) == 0
    # nothing outside [lo, lo + n) (state: outside the groups of the range) changed
    for k in ("param", "master"):
        if c[k] is not None:
            assert torch.equal(c[k][:lo], before[k][:lo]) and torch.equal(c[k][lo + n:], before[k][lo + n:]), k
    assert torch.equal(c["grad"], before["grad"]) and torch.equal(c["mask"], before["mask"])
    cl, ch = (lo, hi) if bits == 8 else (lo // 2, hi // 2)
    for k in ("mq", "vq"):
        assert torch.equal(c[k][:cl], before[k][:cl]) and torch.equal(c[k][ch:], before[k][ch:]), k
    for k in ("ms", "vs"):
        assert torch.equal(c[k][:lo // 128], before[k][:lo // 128]), k
        assert torch.equal(c[k][hi // 128:], before[k][hi // 128:]), k


@functools.lru_cache(maxsize=None)
def _stepped(bits, n, lo):
    """(inputs, outputs of one kernel step) of the standard case -- shared, read only."""
    before = _inputs(bits, n, lo)
    c = _clone(before)
    assert _launch(c, bits, n, lo) == 0
    torch.cuda.synchronize()
    return before, c


SHAPES = [(64, 0), (128 * 3 + 64, 0), (300, 0), (128 * 40 + 77, 0), (1 << 16, 4096), (1 << 22, 0)]


@pytest.mark.parametrize("n,lo", SHAPES)
@pytest.mark.parametrize("bits", [8, 4])
def test_kernel_step_matches_fp32_reference(bits, n, lo):
    before, c = _stepped(bits, n, lo)
    _check(c, before, _reference(before, bits, n, lo), bits, n, lo)


@pytest.mark.parametrize("n,lo", [(300, 0), (128 * 40 + 77, 0), (1 << 16, 4096)])
@pytest.mark.parametrize("bits", [8, 4])
def test_same_decoded_state_gives_dw_adam_flat_bit_for_bit(bits, n, lo):
    """The quantized kernel decodes like the torch codec and updates with the
    adam_elem of the fp32 kernel: master and parameter are bit-identical."""
    from dlrover_wuqiong_amd.ops import _hip

    before, c = _stepped(bits, n, lo)
    m, v = _decode(before, bits, 0, before["param"].numel())
    param, master = before["param"].clone(), before["master"].clone()
    _hip.check(_hip.lib().dw_adam_flat(
        _hip.ptr(param[lo:]), 1, _hip.ptr(master[lo:]), _hip.ptr(before["grad"][lo:]), 1, _hip.ptr(m[lo:]),
        _hip.ptr(v[lo:]), _hip.ptr(before["gs"]), n, 0, HP["lr"], HP["b1"], HP["b2"], HP["eps"], HP["wd"], HP["bc1"],
        HP["bc2"], 1, _hip.ptr(before["mask"][lo // 64:]), _hip.stream()), "adam")
    torch.cuda.synchronize()
    assert torch.equal(master, c["master"])
    assert torch.equal(param, c["param"])


VARIANTS = {
    "fp32_param_no_master_fp32_grad": (dict(pdt=torch.float32, gdt=torch.float32, master=False), {}),
    "adam_l2": ({}, dict(adamw=0)),
    "null_gscale": ({}, dict(gscale=False)),
    "n_decay_prefix": ({}, dict(n_decay=300)),
    "fp32_grad_bf16_param": (dict(gdt=torch.float32), {}),
    "fp32_param_with_master": (dict(pdt=torch.float32), {}),
}


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("bits", [8, 4])
def test_kernel_variants(bits, variant):
    n = 128 * 5 + 64
    ikw, lkw = VARIANTS[variant]
    before = _inputs(bits, n, 0, **ikw)
    c = _clone(before)
    assert _launch(c, bits, n, **lkw) == 0
    _check(c, before, _reference(before, bits, n, **lkw), bits, n)


@pytest.mark.parametrize("bits", [8, 4])
def test_fresh_state_and_zero_gradient_group(bits):
    n = 128 * 5 + 64
    before = _inputs(bits, n, 0, fresh=True, zero_group=2)
    assert all(int(before[k].count_nonzero()) == 0 for k in ("mq", "vq", "ms", "vs"))
    c = _clone(before)
    assert _launch(c, bits, n) == 0
    _check(c, before, _reference(before, bits, n), bits, n)
    # the group whose gradients are all zero: scale 0, codes 0
    assert float(c["ms"][2]) == 0.0 and float(c["vs"][2]) == 0.0
    assert int(_unpack(c["mq"], bits)[256:384].count_nonzero()) == 0
    assert int(_unpack(c["vq"], bits)[256:384].count_nonzero()) == 0
    assert int(c["ms"][:5].count_nonzero()) == 4  # (the others moved)
    for k in ("master", "param", "ms", "vs"):
        assert bool(torch.isfinite(c[k].float()).all()), k
    # a second step from that state (scale-0 group included) stays finite and right
    before2 = _clone(c)
    assert _launch(c, bits, n) == 0
    _check(c, before2, _reference(before2, bits, n), bits, n)


@pytest.mark.parametrize("bits", [8, 4])
def test_split_equals_whole_and_runs_repeat(bits):
    n, cut = 128 * 40 + 77, 128 * 13
    before, whole = _stepped(bits, n, 0)
    again, split = _clone(before), _clone(before)
    assert _launch(again, bits, n) == 0
    assert _launch(split, bits, cut, 0) == 0 and _launch(split, bits, n - cut, cut) == 0
    torch.cuda.synchronize()
    for k in ("param", "master", "mq", "vq", "ms", "vs"):
        assert torch.equal(again[k], whole[k]), k
        assert torch.equal(split[k], whole[k]), k


def test_invalid_arguments_launch_nothing():
    n = 128 * 5 + 64
    before = _inputs(8, n, 0)
    c = _clone(before)
    assert _launch(c, 3, n) != 0
    c["master"] = None  # a bf16 parameter without master
    assert _launch(c, 8, n) != 0
    c["master"] = before["master"].clone()
    assert _launch(c, 8, 0) == 0  # n == 0: nothing to do
    torch.cuda.synchronize()
    for k, v in before.items():
        assert torch.equal(c[k], v), k


# ------------------------------------------------------------ the optimizer
def _gpt2_tiny(device, seed=0):
    from dlrover_wuqiong_amd.models.gpt2 import GPT2, GPT2Config
    from dlrover_wuqiong_amd.parallel.flat import FlatParams

    torch.manual_seed(seed)
    cfg = GPT2Config.named("gpt2-tiny")
    with torch.device(device):
        model = GPT2(cfg)
    model.to(torch.bfloat16)
    return model, FlatParams(model), cfg


def _rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


@pytest.mark.parametrize("bits", [8, 4])
def test_three_optimizer_steps_match_the_cpu_path(bits):
    from dlrover_wuqiong_amd.optimizers.fused import FusedQAdamW

    model, flat, cfg = _gpt2_tiny("cuda")
    _cm, cflat, _ = _gpt2_tiny("cpu")
    cflat.data.copy_(flat.data.cpu())
    assert cflat.numel == flat.numel and torch.equal(cflat.decay_mask, flat.decay_mask.cpu())
    kw = dict(lr=1e-3, weight_decay=0.1, q_bits=bits, max_grad_norm=1.0)
    opt, copt = FusedQAdamW(flat, **kw), FusedQAdamW(cflat, **kw)
    assert torch.equal(copt.master, opt.master.cpu())
    g = torch.Generator().manual_seed(1)
    for _ in range(3):
        x = torch.randint(0, cfg.vocab_size, (2, 65), generator=g).cuda()
        model(x[:, :-1], x[:, 1:]).backward()
        opt.step()
        cflat.grad.copy_(flat.grad.cpu())  # (after the step's pre-hook has completed the gradient)
        copt.step()
        flat.zero_grad()
    torch.cuda.synchronize()
    assert opt.step_count == 3
    assert float(opt.last_grad_norm) == pytest.approx(float(copt.last_grad_norm), rel=1e-3)
    assert _rel(opt.master, copt.master) < 2e-3
    assert _rel(opt.decode_moments()[0], copt.decode_moments()[0]) < 2e-2


def test_flash_checkpoint_round_trip_in_place(tmp_path):
    from dlrover_wuqiong_amd.flash_checkpoint.checkpointer import StorageType
    from dlrover_wuqiong_amd.flash_checkpoint.ddp import DdpCheckpointer
    from dlrover_wuqiong_amd.optimizers.fused import FusedQAdamW

    def make():
        model, flat, cfg = _gpt2_tiny("cuda")
        opt = FusedQAdamW(flat, lr=1e-3, q_bits=8)
        x = torch.randint(0, cfg.vocab_size, (2, 65), generator=torch.Generator().manual_seed(2)).cuda()
        model(x[:, :-1], x[:, 1:]).backward()
        opt.step()
        return model, flat, opt

    model, flat, opt = make()
    _tm, tflat, twin = make()
    bufs = lambda o: (*o._qbuffers().values(), o.master)  # noqa
    # the twin: the same parameters, gradient and optimizer state, never disturbed
    for a, b in zip((tflat.data, tflat.grad, *bufs(twin)), (flat.data, flat.grad, *bufs(opt))):
        a.copy_(b)
    ck = DdpCheckpointer(str(tmp_path / "ck"))
    state = lambda: {"model": model.state_dict(), "opt": opt.state_dict()}  # noqa
    try:
        assert ck.save_checkpoint(5, state(), storage_type=StorageType.MEMORY)
        ck.wait_latest_checkpoint()
        ref = [t.clone() for t in bufs(opt)]
        ptrs = [t.data_ptr() for t in bufs(opt)]
        opt.exp_avg_q.fill_(7)
        opt.exp_avg_sq_q.fill_(9)
        opt.exp_avg_scale.fill_(3.0)
        opt.exp_avg_sq_scale.fill_(-1.0)
        opt.master.zero_()
        opt.step_count = 0
        ck.load_checkpoint(target=state())
        torch.cuda.synchronize()
        assert [t.data_ptr() for t in bufs(opt)] == ptrs
        for a, b in zip(bufs(opt), ref):
            assert torch.equal(a, b)
        assert opt.step_count == 1
    finally:
        ck.close()
    # the next step equals the undisturbed twin's, bit for bit (same gradient: the one of the first backward)
    opt.step()
    twin.step()
    torch.cuda.synchronize()
    for a, b in zip((flat.data, *bufs(opt)), (tflat.data, *bufs(twin))):
        assert torch.equal(a, b)


def test_auto_accelerate_flat_zero2_with_q_adamw():
    from dlrover_wuqiong_amd.atorch.auto_accelerate import auto_accelerate
    from dlrover_wuqiong_amd.models.llama import Llama, LlamaConfig, LlamaDecoderLayer
    from dlrover_wuqiong_amd.optimizers.fused import FusedQAdamW
    from dlrover_wuqiong_amd.optimizers.low_bit import Q_AdamW
    from dlrover_wuqiong_amd.parallel.flat_fsdp import FlatFSDP

    torch.manual_seed(0)
    cfg = LlamaConfig.named("llama-tiny")
    with torch.device("cuda"):
        m = Llama(cfg)
    ok, res, _ = auto_accelerate(m, Q_AdamW, optim_args={"lr": 1e-3, "q_bits": 8, "max_grad_norm": 1.0},
                                 load_strategy=["module_replace", "half",
                                                ("flat_zero2", {"wrap_cls": (LlamaDecoderLayer,)})])
    assert ok and isinstance(res.model, FlatFSDP)
    model, opt = res.model, res.optim
    assert isinstance(opt, FusedQAdamW) and opt.q_bits == 8 and opt.flat is model.shard_flat
    g = torch.Generator().manual_seed(3)
    w0 = opt.master.clone()
    for _ in range(2):
        x = torch.randint(0, cfg.vocab_size, (2, 129), generator=g).cuda()
        loss = model(x[:, :-1], x[:, 1:])
        loss.backward()
        opt.step()
        opt.zero_grad()
        assert bool(torch.isfinite(loss))
    torch.cuda.synchronize()
    assert opt.step_count == 2 and int(opt.exp_avg_q.count_nonzero()) > 0
    assert bool(torch.isfinite(opt.master).all()) and not torch.equal(opt.master, w0)
