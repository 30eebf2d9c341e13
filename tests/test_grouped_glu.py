"""Fused SwiGLU expert projection (``grouped_swiglu_linear``) on CPU tensors:
the reference math, and the ``fused_glu`` / ``fused_experts`` /
``moe_fused_experts`` flag plumbing down to ``Experts``."""

import pytest
import torch
import torch.nn.functional as F


def _explicit(x, w1, w3, counts):
    outs, off = [], 0
    for e, n in enumerate(counts):
        xe = x[off:off + n]
        outs.append(F.silu(xe @ w1[e].t()) * (xe @ w3[e].t()))
        off += n
    return torch.cat(outs, 0)


@pytest.mark.parametrize("counts", [[3, 0, 5, 1], [0, 0, 7], [4]])
def test_grouped_swiglu_linear_cpu_matches_explicit(counts):
    from dlrover_wuqiong_amd.ops.grouped_gemm import grouped_swiglu_linear, offsets_from_counts

    torch.manual_seed(0)
    E, T, H, Fd = len(counts), sum(counts), 16, 24
    x = torch.randn(T, H, dtype=torch.float64, requires_grad=True)
    w1 = torch.randn(E, Fd, H, dtype=torch.float64, requires_grad=True)
    w3 = torch.randn(E, Fd, H, dtype=torch.float64, requires_grad=True)
    offs = offsets_from_counts(counts, "cpu")
    h = grouped_swiglu_linear(x, w1, w3, offs)
    xr, w1r, w3r = (t.detach().clone().requires_grad_() for t in (x, w1, w3))
    hr = _explicit(xr, w1r, w3r, counts)
    assert h.shape == (T, Fd)
    torch.testing.assert_close(h, hr, rtol=1e-12, atol=1e-12)
    dh = torch.randn_like(h)
    h.backward(dh)
    hr.backward(dh)
    for a, b in ((x, xr), (w1, w1r), (w3, w3r)):
        torch.testing.assert_close(a.grad, b.grad, rtol=1e-12, atol=1e-12)
    for e, c in enumerate(counts):
        if c == 0:
            assert w1.grad[e].abs().max() == 0 and w3.grad[e].abs().max() == 0


def test_grouped_swiglu_linear_cpu_no_rows():
    from dlrover_wuqiong_amd.ops.grouped_gemm import grouped_swiglu_linear, offsets_from_counts

    E, H, Fd = 3, 16, 8
    x = torch.zeros(0, H, requires_grad=True)
    w1 = torch.randn(E, Fd, H, requires_grad=True)
    w3 = torch.randn(E, Fd, H, requires_grad=True)
    h = grouped_swiglu_linear(x, w1, w3, offsets_from_counts([0] * E, "cpu"))
    assert h.shape == (0, Fd)
    h.sum().backward()
    assert w1.grad is not None and w1.grad.shape == w1.shape and w1.grad.abs().max() == 0
    assert w3.grad is not None and w3.grad.shape == w3.shape and w3.grad.abs().max() == 0


@pytest.mark.parametrize("capacity_factor", [0.0, 1.0])
def test_moe_layer_fused_experts_cpu_bitwise(capacity_factor):
    from dlrover_wuqiong_amd.parallel.moe import MoELayer

    torch.manual_seed(1)
    H, Fd, E = 32, 48, 4
    a = MoELayer(H, Fd, E, top_k=2, capacity_factor=capacity_factor, fused_experts=False)
    b = MoELayer(H, Fd, E, top_k=2, capacity_factor=capacity_factor, fused_experts=True)
    b.load_state_dict(a.state_dict())
    assert b.experts.fused_glu is True and a.experts.fused_glu is False
    x = torch.randn(2, 9, H)
    xa, xb = x.clone().requires_grad_(), x.clone().requires_grad_()
    ya, yb = a(xa), b(xb)
    assert torch.equal(ya, yb)
    (ya.pow(2).mean() + a.aux_loss).backward()
    (yb.pow(2).mean() + b.aux_loss).backward()
    assert torch.equal(xa.grad, xb.grad)
    for (n, p), (_, q) in zip(a.named_parameters(), b.named_parameters()):
        assert p.grad is not None and torch.equal(p.grad, q.grad), n


def test_grouped_mlp_fused_flag_leaves_other_paths_alone():
    from dlrover_wuqiong_amd.parallel.moe import grouped_mlp

    torch.manual_seed(2)
    counts, H, Fd = [2, 0, 3], 16, 24
    x = torch.randn(sum(counts), H)
    w1, w3, w2 = torch.randn(3, Fd, H), torch.randn(3, Fd, H), torch.randn(3, H, Fd)
    for w3_, act in ((w3, "silu"), (w3, "gelu"), (None, "silu"), (None, "gelu")):
        assert torch.equal(grouped_mlp(x, counts, w1, w2, w3_, act, fused_glu=True),
                           grouped_mlp(x, counts, w1, w2, w3_, act))


def test_llama_config_moe_fused_experts_reaches_experts():
    from dlrover_wuqiong_amd.models.llama import Llama, LlamaConfig
    from dlrover_wuqiong_amd.parallel.moe import Experts

    assert LlamaConfig().moe_fused_experts is False
    base = LlamaConfig.named("llama-moe-tiny")
    for flag in (False, True):
        cfg = LlamaConfig(**{**base.__dict__, "num_hidden_layers": 1, "moe_fused_experts": flag})
        experts = [m for m in Llama(cfg).modules() if isinstance(m, Experts)]
        assert experts and all(m.fused_glu is flag for m in experts)


def test_replace_with_moe_passes_fused_experts():
    import torch.nn as nn

    from dlrover_wuqiong_amd.parallel.moe import MoELayer, replace_with_moe

    class FFN(nn.Module):
        def __init__(self):
            super().__init__()
            self.gate_proj = nn.Linear(16, 24, bias=False)
            self.up_proj = nn.Linear(16, 24, bias=False)
            self.down_proj = nn.Linear(24, 16, bias=False)

    model = nn.Sequential(FFN(), FFN())
    assert len(replace_with_moe(model, FFN, 4, fused_experts=True)) == 2
    assert all(isinstance(m, MoELayer) and m.experts.fused_glu for m in model)
