"""FusedQAdamW (flat fused AdamW with 8-/4-bit block-quantized moments): the
CPU reference path, the state dict and the wiring.  The HIP kernel is checked
against this path in test_qadam_flat_gpu.py."""

import math

import pytest
import torch

BITS = (8, 4)


def _mlp(dtype=torch.float32, seed=0, hidden=72):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(24, hidden), torch.nn.Tanh(), torch.nn.Linear(hidden, 3)).to(dtype)


def _problem(seed=0):
    torch.manual_seed(seed)
    model = torch.nn.Sequential(torch.nn.Linear(32, 64), torch.nn.Tanh(), torch.nn.Linear(64, 1))
    x = torch.randn(256, 32)
    y = (x[:, :4].sum(1, keepdim=True)).tanh()
    return model, x, y


def test_construction_allocates_no_fp32_moments():
    from dlrover_wuqiong_amd.optimizers.fused import FusedQAdamW
    from dlrover_wuqiong_amd.parallel.flat import FlatParams

    for bits in BITS:
        flat = FlatParams(_mlp())
        opt = FusedQAdamW(flat, q_bits=bits)
        n = flat.numel
        assert not hasattr(opt, "exp_avg") and not hasattr(opt, "exp_avg_sq")
        assert not any(torch.is_tensor(v) and v.dtype == torch.float32 and v.numel() == n
                       for v in vars(opt).values())  # fp32 parameters: no master either
        npad = (n + 127) // 128 * 128
        assert opt.exp_avg_q.dtype == torch.uint8 and opt.exp_avg_q.numel() == (npad if bits == 8 else npad // 2)
        assert opt.exp_avg_sq_q.numel() == opt.exp_avg_q.numel()
        assert opt.exp_avg_scale.dtype == torch.float32 and opt.exp_avg_scale.numel() == npad // 128
        assert opt.exp_avg_sq_scale.numel() == npad // 128
        assert all(int(t.count_nonzero()) == 0 for t in opt._qbuffers().values())
        assert opt.step_count == 0 and not opt._dsw_supported()
    with pytest.raises(ValueError):
        FusedQAdamW(FlatParams(_mlp()), q_bits=3)


@pytest.mark.parametrize("bits,bound", [(8, 0.5), (4, 0.45)])
def test_state_bytes_against_fused_adamw(bits, bound):
    """``state_bytes()`` (as ``Q_AdamW.state_bytes``: the codes and scales of
    the two moments, no copy of the weights) against the bytes FusedAdamW holds
    for the same bf16 model with master (exp_avg + exp_avg_sq + master, 12 B
    per element).

    The byte counts follow from the formats, so they are asserted exactly: per
    128-element group 2 * 128 * bits / 8 bytes of codes and two fp32 scales.
    With the 4 B of master that both optimizers hold, the quantized one keeps
    (4 + 2 * bits / 8 + 1 / 16) / 12 of FusedAdamW's bytes resident: 0.5052 at
    8 bits (above one half by the scales), 0.4219 at 4 bits."""
    from dlrover_wuqiong_amd.optimizers.fused import FusedAdamW, FusedQAdamW
    from dlrover_wuqiong_amd.parallel.flat import FlatParams

    ref = FusedAdamW(FlatParams(_mlp(torch.bfloat16)))
    ref_bytes = sum(t.numel() * t.element_size() for t in (ref.exp_avg, ref.exp_avg_sq, ref.master))
    opt = FusedQAdamW(FlatParams(_mlp(torch.bfloat16)), q_bits=bits)
    assert opt.master is not None and opt.master.dtype == torch.float32
    ratio = opt.state_bytes() / ref_bytes
    print(f"q_bits={bits}: state_bytes {opt.state_bytes()} / {ref_bytes} = {ratio:.4f}")
    assert ratio < bound, (bits, ratio)
    n = opt.flat.numel
    assert n % 128 == 0 and ref_bytes == 12 * n
    assert opt.state_bytes() == n // 128 * (2 * 128 * bits // 8 + 8)
    resident = opt.state_bytes() + opt.master.numel() * 4
    assert resident / ref_bytes == pytest.approx((4 + 2 * bits / 8 + 1 / 16) / 12, rel=1e-12)


def _reference_step(bits, w, g, mq, vq, ms, vs, decay, n, lr, b1, b2, eps, wd, t, max_norm, adamw=True):
    """decode -> fp32 AdamW -> encode, written out by hand with the low_bit codec."""
    from dlrover_wuqiong_amd.optimizers import low_bit as lb

    npad = (n + 127) // 128 * 128
    G = npad // 128
    mc = lb._unpack4(mq) if bits == 4 else mq
    vc = lb._unpack4(vq) if bits == 4 else vq
    m = lb.dequant_m(mc.view(G, 128), ms, bits).reshape(-1).clone()
    v = lb.dequant_v(vc.view(G, 128), vs, bits).reshape(-1).clone()
    g = g.float()
    nrm = float((g * g).sum().sqrt())
    g = g * min(1.0, max_norm / (nrm + 1e-6)) if max_norm > 0 else g
    w = w.clone()
    if not adamw:
        g = g + wd * w * decay
    m[:n] = m[:n] * b1 + (1 - b1) * g
    v[:n] = v[:n] * b2 + (1 - b2) * g * g
    m[n:] = 0
    v[n:] = 0
    bc1, bc2 = 1 - b1 ** t, 1 - b2 ** t
    denom = v[:n].sqrt() / math.sqrt(bc2) + eps
    if adamw:
        w = w - lr * wd * w * decay
    w = w - (lr / bc1) * m[:n] / denom
    mcodes, ms2 = lb.quant_m(m.view(G, 128), bits)
    vcodes, vs2 = lb.quant_v(v.view(G, 128), bits)
    pk = (lambda c: lb._pack4(c.reshape(-1))) if bits == 4 else (lambda c: c.reshape(-1))
    return w, pk(mcodes), pk(vcodes), ms2, vs2


@pytest.mark.parametrize("adamw", [True, False])
@pytest.mark.parametrize("bits", BITS)
def test_cpu_step_equals_handwritten_reference(bits, adamw):
    from dlrover_wuqiong_amd.optimizers.fused import FusedQAdamW
    from dlrover_wuqiong_amd.parallel.flat import FlatParams

    # weight 72x24 = 1728 (27 blocks of 64: decays), bias 72 (-> 128, no decay), weight 3x72 = 216 (-> 256),
    # bias 3 (-> 64): numel = 2176 = 17 * 128: make it 64 mod 128 with one more no-decay vector
    model = _mlp()
    model.register_parameter("extra", torch.nn.Parameter(torch.randn(40)))
    flat = FlatParams(model)
    n = flat.numel
    assert n % 128 == 64
    dm = flat.decay_mask.view(-1)
    pairs = dm[: n // 128 * 2].view(-1, 2)
    assert bool((pairs[:, 0] != pairs[:, 1]).any())  # a 128-group holding a decayed and an undecayed block
    lr, b1, b2, eps, wd, max_norm = 3e-3, 0.9, 0.95, 1e-8, 0.1, 0.5
    opt = FusedQAdamW(flat, lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, q_bits=bits, max_grad_norm=max_norm,
                      adamw=adamw)
    decay = dm.repeat_interleave(64)[:n].bool()
    gen = torch.Generator().manual_seed(5)
    for t in (1, 2, 3):
        flat.grad.copy_(torch.randn(n, generator=gen) * (1.0 + 3.0 * (torch.arange(n) % 7 == 0)))
        want = _reference_step(bits, flat.data, flat.grad, opt.exp_avg_q, opt.exp_avg_sq_q, opt.exp_avg_scale,
                               opt.exp_avg_sq_scale, decay, n, lr, b1, b2, eps, wd, t, max_norm, adamw)
        opt.step()
        assert opt.step_count == t
        torch.testing.assert_close(flat.data, want[0], rtol=1e-6, atol=1e-7)
        assert torch.equal(opt.exp_avg_q, want[1]) and torch.equal(opt.exp_avg_sq_q, want[2])
        torch.testing.assert_close(opt.exp_avg_scale, want[3], rtol=1e-6, atol=0)
        torch.testing.assert_close(opt.exp_avg_sq_scale, want[4], rtol=1e-6, atol=0)
        assert float(opt.last_grad_norm) == pytest.approx(float(flat.grad.norm()), rel=1e-5)
    # the half-filled last group: padding codes stay 0
    pad = slice(n, None) if bits == 8 else slice(n // 2, None)
    assert int(opt.exp_avg_q[pad].count_nonzero()) == 0 and int(opt.exp_avg_sq_q[pad].count_nonzero()) == 0
    assert int(opt.exp_avg_q.count_nonzero()) > n // 4  # (and the rest is in use)


def test_trains_close_to_fused_adamw():
    from dlrover_wuqiong_amd.optimizers.fused import FusedAdamW, FusedQAdamW
    from dlrover_wuqiong_amd.parallel.flat import FlatParams

    for bits in (4, 8):
        model, x, y = _problem()
        ref_model = _problem()[0]
        opt = FusedQAdamW(FlatParams(model), lr=1e-2, weight_decay=0.0, q_bits=bits)
        ref = FusedAdamW(FlatParams(ref_model), lr=1e-2, weight_decay=0.0)
        for _ in range(60):
            for m, o in ((model, opt), (ref_model, ref)):
                o.zero_grad()
                torch.nn.functional.mse_loss(m(x), y).backward()
                o.step()
        with torch.no_grad():
            lq = float(torch.nn.functional.mse_loss(model(x), y))
            l_ref = float(torch.nn.functional.mse_loss(ref_model(x), y))
        assert lq < 0.05 and lq < 3 * l_ref + 0.01, (bits, lq, l_ref)


def _fill_grads(flat, gen):
    # through the parameters' views: the alignment padding between them keeps a zero gradient
    for p in flat.params:
        p.grad.copy_(torch.randn(p.shape, generator=gen).to(p.grad.dtype))


def _stepped(bits, dtype, steps=2, seed=3):
    from dlrover_wuqiong_amd.optimizers.fused import FusedQAdamW
    from dlrover_wuqiong_amd.parallel.flat import FlatParams

    flat = FlatParams(_mlp(dtype))
    opt = FusedQAdamW(flat, lr=1e-2, q_bits=bits, max_grad_norm=1.0)
    gen = torch.Generator().manual_seed(seed)
    for _ in range(steps):
        _fill_grads(flat, gen)
        opt.step()
    return flat, opt


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("bits", BITS)
def test_state_dict_round_trip(bits, dtype):
    from dlrover_wuqiong_amd.optimizers.fused import FusedAdamW, FusedQAdamW
    from dlrover_wuqiong_amd.parallel.flat import FlatParams

    flat, opt = _stepped(bits, dtype)
    sd = opt.state_dict()
    q = sd["quantized"]
    assert q["q_bits"] == bits and q["group"] == 128
    for k in ("exp_avg_q", "exp_avg_sq_q", "exp_avg_scale", "exp_avg_sq_scale"):
        assert q[k].data_ptr() == getattr(opt, k).data_ptr() and q[k].numel() == getattr(opt, k).numel()
    assert set(sd["state"]) == set(range(len(flat.params)))
    for i, (o, c) in enumerate(flat.offsets):
        s = sd["state"][i]
        assert float(s["step"]) == 2 and "exp_avg" not in s
        if dtype == torch.bfloat16:
            assert s["master_param"].data_ptr() == opt.master[o:o + c].data_ptr()
            assert s["master_param"].shape == flat.params[i].shape
        else:
            assert "master_param" not in s
    assert sd["param_groups"][0]["lr"] == 1e-2
    # loading an optimizer's own state dict copies nothing onto itself
    opt.load_state_dict(sd)

    flat2 = FlatParams(_mlp(dtype, seed=9))
    opt2 = FusedQAdamW(flat2, lr=5e-2, q_bits=bits, max_grad_norm=1.0)
    flat2.data.copy_(flat.data)
    opt2.load_state_dict(sd)
    assert opt2.step_count == 2 and opt2.param_groups[0]["lr"] == 1e-2
    for f, o in ((flat, opt), (flat2, opt2)):
        _fill_grads(f, torch.Generator().manual_seed(11))
        o.step()
    assert torch.equal(flat.data, flat2.data)
    for k, t in opt._qbuffers().items():
        assert torch.equal(t, opt2._qbuffers()[k]), k
    if opt.master is not None:
        assert torch.equal(opt.master, opt2.master)

    # mismatches raise
    other = FusedQAdamW(FlatParams(_mlp(dtype)), q_bits=12 - bits)
    with pytest.raises(ValueError, match="q_bits"):
        other.load_state_dict(sd)
    longer = FusedQAdamW(FlatParams(_mlp(dtype, hidden=80)), q_bits=bits)
    with pytest.raises(ValueError, match="exp_avg_q"):
        longer.load_state_dict(sd)
    fp32_sd = FusedAdamW(FlatParams(_mlp(dtype))).state_dict()
    with pytest.raises(ValueError, match="exp_avg"):
        FusedQAdamW(FlatParams(_mlp(dtype)), q_bits=bits).load_state_dict(fp32_sd)


def test_overlap_with_forward_is_refused():
    from dlrover_wuqiong_amd.optimizers.fused import FusedQAdamW
    from dlrover_wuqiong_amd.parallel.flat import FlatParams

    model = _mlp()
    opt = FusedQAdamW(FlatParams(model))
    with pytest.raises(NotImplementedError, match="128"):
        opt.overlap_with_forward(model)


def test_checkpoint_safe_tensors_lists_the_quantized_state():
    _flat, opt = _stepped(8, torch.bfloat16, steps=1)
    got = {t.data_ptr() for t in opt.checkpoint_safe_tensors()}
    want = (opt.flat.data, opt.exp_avg_q, opt.exp_avg_sq_q, opt.exp_avg_scale, opt.exp_avg_sq_scale, opt.master)
    assert got == {t.data_ptr() for t in want} and len(opt.checkpoint_safe_tensors()) == 6


def _flat_fsdp():
    from dlrover_wuqiong_amd.models.gpt2 import GPT2, Block, GPT2Config
    from dlrover_wuqiong_amd.parallel.flat_fsdp import FlatFSDP

    torch.manual_seed(0)
    return FlatFSDP(GPT2(GPT2Config.named("gpt2-tiny")), wrap_cls=(Block,))


def test_flat_optimizer_builds_fused_qadamw_for_q_adamw():
    from dlrover_wuqiong_amd.atorch.auto_accelerate import _flat_optimizer
    from dlrover_wuqiong_amd.optimizers.fused import FusedAdamW, FusedQAdamW
    from dlrover_wuqiong_amd.optimizers.low_bit import Q_AdamW

    fs = _flat_fsdp()
    opt = _flat_optimizer(fs, Q_AdamW, {"lr": 2e-3, "betas": (0.8, 0.9), "eps": 1e-6, "weight_decay": 0.2,
                                        "max_grad_norm": 1.5, "q_bits": 4, "threshold": 1})
    assert isinstance(opt, FusedQAdamW) and opt.flat is fs.shard_flat and opt.q_bits == 4
    g = opt.param_groups[0]
    assert (g["lr"], g["betas"], g["eps"], g["weight_decay"]) == (2e-3, (0.8, 0.9), 1e-6, 0.2)
    assert opt.max_grad_norm == 1.5
    assert _flat_optimizer(fs, FusedQAdamW, {}).q_bits == 8
    assert type(_flat_optimizer(fs, torch.optim.AdamW, {"lr": 1e-3})) is FusedAdamW
    with pytest.raises(ValueError, match="Q_AdamW"):
        _flat_optimizer(fs, torch.optim.SGD, {})


def test_get_fsdp_optim_param_refuses_the_quantized_optimizer():
    from dlrover_wuqiong_amd.atorch import fsdp_flat_ckpt as ffc
    from dlrover_wuqiong_amd.optimizers.fused import FusedAdamW, FusedQAdamW

    fs = _flat_fsdp()
    with pytest.raises(NotImplementedError, match=r"state_dict\(\).*DdpCheckpointer.*[Rr]esharding"):
        ffc.get_fsdp_optim_param(fs, FusedQAdamW(fs.shard_flat))
    states, _groups = ffc.get_fsdp_optim_param(fs, FusedAdamW(fs.shard_flat))  # unchanged for fp32 moments
    assert any(k.endswith("-exp_avg") for k in states)
