"""GPU: ``linear_token_logprobs`` (csrc/kernels/linear_logprob.hip) against
fp64 ``log_softmax(X W^T)``.  ``lse`` is not returned by either path; it is
checked through ``logp = x[label] - lse`` and ``ent = lse - sum p x``."""

import pytest
import torch
import torch.nn.functional as F

from dlrover_wuqiong_amd.ops.token_stats import linear_logprob_splits, linear_token_logprobs, token_logprobs

pytestmark = pytest.mark.gpu

# id: (hidden shape, slice of dim 1 or None, V, row of W scaled by 8 (dominant logit in that tile) or None)
CASES = {
    "one_partial_tile": ((1, 64), None, 127, None),
    "all_tails": ((129, 72), None, 129, -1),
    "odd_k_many_tiles": ((128, 192), None, 128 * 5 + 1, -1),
    "unequal_splits": ((300, 128), None, 128 * 400 + 5, 0),
    "strided_view": ((3, 40, 64), slice(7, -1), 257, 0),
}


@pytest.fixture(scope="module", params=list(CASES), ids=list(CASES))
def case(request):
    shape, sl, V, big = CASES[request.param]
    H = shape[-1]
    g = torch.Generator().manual_seed(len(request.param))
    W = torch.randn(V, H, generator=g) * 3 / H ** 0.5
    if big is not None:
        W[big] *= 8
    full = torch.randn(*shape, generator=g).bfloat16().cuda()
    W = W.bfloat16().cuda()
    X = full if sl is None else full[:, sl, :]
    labels = torch.randint(0, V, X.shape[:-1], generator=g).cuda()
    flat = labels.view(-1)   # first / last row of a tile, V - 1, ignored (rows = 1 keeps V - 1 alone)
    for i, v in enumerate([0, min(127, V - 1), -100, min(128, V - 1), V - 1][-flat.numel():]):
        flat[i] = v
    x64 = X.double() @ W.double().T
    lp64 = x64.log_softmax(-1)
    valid = labels >= 0
    ref = (torch.where(valid, lp64.gather(-1, labels.clamp(min=0).unsqueeze(-1)).squeeze(-1), 0.0),
           -(lp64.exp() * lp64).sum(-1))
    err = lambda out: max(float((o.double() - r).abs().max()) for o, r in zip(out, ref))  # noqa: E731
    # fp32 accumulation in any order, doubled for x[label] - lse
    acc_bound = 2 * H * 2.0 ** -24 * float((X.double().abs() @ W.double().abs().T).max())
    # what __expf / logf and the fp32 sums cost the existing statistics kernel on fp32 logits, no GEMM
    slack = 4 * err(token_logprobs(x64.float(), labels, True))
    return dict(name=request.param, X=X, W=W, labels=labels, V=V, err=err, bound=acc_bound + slack, slack=slack,
                today=err(token_logprobs(F.linear(X, W), labels, True)))


def test_against_fp64(case):
    X, W, labels = case["X"], case["W"], case["labels"]
    out = linear_token_logprobs(X, W, labels, True)
    e = case["err"](out)
    print(f"{case['name']}: fused err {e:.3e}, today {case['today']:.3e}, bound {case['bound']:.3e} "
          f"(slack {case['slack']:.3e}), splits {linear_logprob_splits(labels.numel(), case['V'])}")
    assert out[0].dtype == torch.float32 and out[0].shape == labels.shape == out[1].shape
    assert e <= case["today"]
    assert e <= case["bound"]
    assert bool((out[0][labels < 0] == 0).all()) and int((labels < 0).sum()) == (labels.numel() > 1)
    # run to run, and whatever is asked for
    again = linear_token_logprobs(X, W, labels, True)
    assert torch.equal(again[0], out[0]) and torch.equal(again[1], out[1])
    assert torch.equal(linear_token_logprobs(X, W, labels), out[0])
    none = linear_token_logprobs(X, W, None, True)
    assert torch.equal(none[1], out[1]) and not none[0].any()
    if case["name"] == "unequal_splits":
        splits, tiles = linear_logprob_splits(labels.numel(), case["V"]), (case["V"] + 127) // 128
        assert splits >= 2 and tiles % splits


def test_no_logits_sized_allocation():
    rows, H, V = 2048, 64, 32768
    X = torch.randn(rows, H, device="cuda").bfloat16()
    W = (torch.randn(V, H, device="cuda") * 3 / 8).bfloat16()
    labels = torch.randint(0, V, (rows,), device="cuda")
    linear_token_logprobs(X, W, labels, True)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = linear_token_logprobs(X, W, labels, True)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    assert rise < rows * V // 4, rise   # an eighth of the bf16 logits
    assert torch.isfinite(out[0]).all()
