"""GPU: the token log-prob / entropy kernels against the fp32 torch
expressions, and the fused sampler: exact membership in the CPU-computed kept
set, the drawn distribution, determinism, graph capture, and generation with
in-graph sampling."""

import functools

import pytest
import torch
import torch.nn.functional as F
from test_rl_token_ops import CASES, HEAD_IDX, MARGIN, V, brute_force, fixture_logits

from dlrover_wuqiong_amd.ops.sampling import keep_mask, sample_tokens
from dlrover_wuqiong_amd.ops.token_stats import token_entropy, token_logprobs

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float32]


def _rel(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def _close_rows(got, ref):
    err = (got.float() - ref).abs()
    assert bool((err <= 1e-3 * ref.abs().clamp_min(1.0)).all()), float(err.max())


def _ref_stats(xf, labels):
    """The fp32 torch expressions (a -inf logit adds 0 to the entropy, a
    label outside [0, V) gives 0)."""
    lp = F.log_softmax(xf, dim=-1)
    valid = (labels >= 0) & (labels < xf.shape[-1])
    logp = lp.gather(-1, labels.clamp(0, xf.shape[-1] - 1).unsqueeze(-1)).squeeze(-1)
    logp = torch.where(valid, logp, torch.zeros_like(logp))
    ent = -(lp.exp() * lp.masked_fill(lp == float("-inf"), 0.0)).sum(-1)
    return logp, ent


def _check_stats(x, labels, with_entropy=True, grad_tol=None):
    """Forward values and the gradients for (g_logp, g_ent) both, one, the
    other, against fp32 autograd on the same values.  ``x`` may be a view."""
    grad_tol = grad_tol or (2e-2 if x.dtype == torch.bfloat16 else 1e-3)
    base = x._base if x._base is not None else x
    leaf = base.detach().clone().requires_grad_()
    view = leaf.as_strided(x.shape, x.stride(), x.storage_offset())
    rleaf = base.detach().float().requires_grad_()
    rview = rleaf.as_strided(x.shape, x.stride(), x.storage_offset())
    ref_logp, ref_ent = _ref_stats(rview, labels)
    if with_entropy:
        logp, ent = token_logprobs(view, labels, with_entropy=True)
        assert ent.dtype == torch.float32 and ent.shape == labels.shape
        _close_rows(ent, ref_ent.detach())
    else:
        logp, ent = token_logprobs(view, labels), None
    assert logp.dtype == torch.float32 and logp.shape == labels.shape
    _close_rows(logp, ref_logp.detach())
    torch.manual_seed(5)
    g1 = torch.randn(labels.shape, device=DEV)
    g2 = torch.randn(labels.shape, device=DEV)
    combos = ((g1, g2), (g1, None), (None, g2)) if with_entropy else ((g1, None),)
    for a, b in combos:
        obj = (0 if a is None else (a * logp).sum()) + (0 if b is None else (b * ent).sum())
        robj = (0 if a is None else (a * ref_logp).sum()) + (0 if b is None else (b * ref_ent).sum())
        got, = torch.autograd.grad(obj, leaf, retain_graph=True)
        ref, = torch.autograd.grad(robj, rleaf, retain_graph=True)
        assert got.dtype == x.dtype and got.shape == base.shape
        assert bool(torch.isfinite(got).all())
        assert _rel(got, ref) < grad_tol, (_rel(got, ref), a is None, b is None)


@pytest.mark.parametrize("with_entropy", [True, False])
@pytest.mark.parametrize("Vv", [8, 1000, 1003, 50257])
@pytest.mark.parametrize("dtype", DTYPES)
def test_token_logprobs_sliced_view(dtype, Vv, with_entropy):
    torch.manual_seed(Vv)
    full = (3 * torch.randn(2, 5, Vv, device=DEV)).to(dtype)
    x = full[:, 1:-1]
    assert not x.is_contiguous()
    labels = torch.randint(0, Vv, (2, 3), device=DEV)
    _check_stats(x, labels, with_entropy)


@pytest.mark.parametrize("dtype", DTYPES)
def test_token_logprobs_llama3_vocab(dtype):
    torch.manual_seed(0)
    x = (3 * torch.randn(2, 128256, device=DEV)).to(dtype)
    labels = torch.tensor([0, 128255], device=DEV)
    _check_stats(x, labels)


@pytest.mark.parametrize("dtype", DTYPES)
def test_token_logprobs_masked_peaked_and_ignored_rows(dtype):
    torch.manual_seed(1)
    Vv = 1003
    x = (2 * torch.randn(4, Vv, device=DEV)).to(dtype)
    x[0, ::3] = float("-inf")          # a third of the vocabulary masked
    x[1, 17] = x[1].float().max() + 60  # one logit 60 above the rest
    labels = torch.tensor([1, 17, -100, 5], device=DEV)  # row 2: ignored label
    logp, ent = token_logprobs(x, labels, with_entropy=True)
    assert bool(torch.isfinite(ent).all()) and bool(torch.isfinite(logp).all())
    assert abs(float(ent[1])) < 1e-3 and abs(float(logp[1])) < 1e-3
    assert float(logp[2]) == 0.0
    _check_stats(x, labels)
    # masked logits get exactly zero gradient
    leaf = x.clone().requires_grad_()
    lp, en = token_logprobs(leaf, labels, with_entropy=True)
    (lp.sum() + en.sum()).backward()
    assert bool((leaf.grad[0, ::3] == 0).all()) and bool(torch.isfinite(leaf.grad).all())


def test_ppo_utils_use_the_op_on_gpu():
    from dlrover_wuqiong_amd.atorch.rl.ppo_utils import (entropy_from_logits, logprobs_and_entropy,
                                                         logprobs_of_labels)

    torch.manual_seed(2)
    full = torch.randn(2, 6, 1000, device=DEV).to(torch.bfloat16)
    x, labels = full[:, 2:-1], torch.randint(0, 1000, (2, 3), device=DEV)
    logp, ent = token_logprobs(x, labels, with_entropy=True)
    assert torch.equal(logprobs_of_labels(x, labels), logp)
    assert torch.equal(entropy_from_logits(x), ent) and torch.equal(token_entropy(x), ent)
    both = logprobs_and_entropy(x, labels)
    assert torch.equal(both[0], logp) and torch.equal(both[1], ent)


# ------------------------------------------------------------------ sampler
N_ROWS = 4096
SEED = 1234


@functools.lru_cache(maxsize=None)
def _kept(Vv, T, top_k, top_p):
    """CPU: (kept indices, renormalised fp64 probabilities over them)."""
    x = fixture_logits(Vv)
    kept, above = brute_force(x, T, top_k, top_p)
    if top_p < 1.0:
        assert float((above - top_p).abs().min()) >= MARGIN
    z = (x.float() / T).double()
    q = torch.where(kept, (z - z.max()).exp(), torch.zeros_like(z))
    return kept, q / q.sum()


def _rows(Vv, dtype):
    return fixture_logits(Vv).to(dtype).to(DEV).unsqueeze(0).repeat(N_ROWS, 1)


def _offset(v=0):
    return torch.full((1,), v, device=DEV, dtype=torch.int64)


@pytest.mark.parametrize("T,top_k,top_p,n_head", CASES)
def test_sampler_membership(T, top_k, top_p, n_head):
    kept, _ = _kept(V, T, top_k, top_p)
    if n_head is not None:
        assert kept.nonzero().view(-1).tolist() == sorted(HEAD_IDX[:n_head])
    x = _rows(V, torch.bfloat16)
    tok = sample_tokens(x, T, top_k, top_p, seed=SEED, offset=_offset())
    assert tok.shape == (N_ROWS, 1) and tok.dtype == torch.int64
    tok = tok.view(-1).cpu()
    assert int(tok.min()) >= 0 and int(tok.max()) < V
    assert bool(kept[tok].all()), sorted(set(tok[~kept[tok]].tolist()))
    # the GPU keep_mask is the same definition
    assert torch.equal(keep_mask(x[:2], T, top_k, top_p).cpu()[0], kept)


@pytest.mark.parametrize("Vv,dtype,T,top_k,top_p", [(1003, torch.bfloat16, 1.0, 0, 0.70),
                                                    (1003, torch.bfloat16, 1.0, 5, 0.90),
                                                    (1003, torch.bfloat16, 1.0, 3, 1.0),
                                                    (V, torch.float32, 1.0, 0, 0.76),
                                                    (V, torch.float32, 0.7, 0, 0.87),
                                                    (V, torch.float32, 1.0, 5, 0.90),
                                                    (V, torch.float32, 1.0, 20, 1.0)])
def test_sampler_membership_unaligned_rows_and_fp32(Vv, dtype, T, top_k, top_p):
    kept, _ = _kept(Vv, T, top_k, top_p)
    x = _rows(Vv, dtype)
    if Vv % 8:
        assert x[1].data_ptr() % 16 != 0
    tok = sample_tokens(x, T, top_k, top_p, seed=SEED, offset=_offset()).view(-1).cpu()
    assert int(tok.min()) >= 0 and int(tok.max()) < Vv
    assert bool(kept[tok].all()), sorted(set(tok[~kept[tok]].tolist()))
    assert len(set(tok.tolist())) > 1


def _within_6_sigma(tok, kept, q, n, pool_rare=False):
    """|count - n q| <= 6 sqrt(n q (1 - q)) + 1 for every kept token.

    ``pool_rare`` (the cases that keep the whole vocabulary): a tail token of
    the fixture has n q = 0.5, where the binomial is far from normal:
    P(count >= 6) is about 1e-5 per token, 5 % over the 4091 of them for an
    exact sampler.  There the tokens with n q < 30 are pooled into one bucket
    (counts and probabilities summed) that is held to the same bound."""
    counts = torch.bincount(tok, minlength=q.numel()).double()
    assert float(counts[~kept].sum()) == 0
    rare = kept & (n * q < 30) if pool_rare else torch.zeros_like(kept)
    qk, ck = q[kept & ~rare], counts[kept & ~rare]
    if bool(rare.any()):
        qk = torch.cat([qk, q[rare].sum().view(1)])
        ck = torch.cat([ck, counts[rare].sum().view(1)])
    bound = 6 * (n * qk * (1 - qk)).sqrt() + 1
    bad = (ck - n * qk).abs() > bound
    assert not bool(bad.any()), (ck[bad].tolist(), (n * qk)[bad].tolist(), bound[bad].tolist())


@pytest.mark.parametrize("T,top_k,top_p", [(1.0, 0, 0.76), (0.7, 0, 0.87), (1.0, 5, 0.90), (1.0, 5, 1.0),
                                           (1.0, 20, 1.0), (1.0, 0, 1.0)])
def test_sampler_distribution(T, top_k, top_p):
    kept, q = _kept(V, T, top_k, top_p)
    pool = bool(kept.all())
    x = _rows(V, torch.bfloat16)
    n = 4 * N_ROWS
    off = _offset()
    tok = torch.cat([sample_tokens(x, T, top_k, top_p, seed=SEED, offset=off) for _ in range(4)]).view(-1).cpu()
    assert int(off) == 4 and tok.numel() == n
    _within_6_sigma(tok, kept, q, n, pool)
    # the bound is loose enough for an exact sampler: torch.multinomial on the same distribution
    torch.manual_seed(SEED)
    ref = torch.multinomial(q.to(DEV).float(), n, replacement=True).cpu()
    _within_6_sigma(ref, kept, q, n, pool)


def test_sampler_is_deterministic_and_offsets_differ():
    x = _rows(V, torch.bfloat16)[:64]
    a = sample_tokens(x, 1.0, 0, 1.0, seed=7, offset=_offset(3))
    b = sample_tokens(x, 1.0, 0, 1.0, seed=7, offset=_offset(3))
    assert torch.equal(a, b)
    assert not torch.equal(a, sample_tokens(x, 1.0, 0, 1.0, seed=7, offset=_offset(4)))
    assert not torch.equal(a, sample_tokens(x, 1.0, 0, 1.0, seed=8, offset=_offset(3)))
    # a row's draw does not depend on its neighbours being there: same (row, offset, B)
    c = sample_tokens(x.float(), 1.0, 50, 0.95, seed=7, offset=_offset(3))
    d = sample_tokens(x.float(), 1.0, 50, 0.95, seed=7, offset=_offset(3))
    assert torch.equal(c, d)
    assert sample_tokens(x, 0.0, seed=7).view(-1).tolist() == [0] * 64  # greedy


def test_sampler_graph_replay_matches_eager():
    x = _rows(V, torch.bfloat16)[:64]
    args = (0.7, 50, 0.87)
    off = _offset()
    eager = [sample_tokens(x, *args, seed=11, offset=off).clone() for _ in range(4)]
    assert int(off) == 4
    goff = _offset()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            out = sample_tokens(x, *args, seed=11, offset=goff)
    torch.cuda.current_stream().wait_stream(s)
    assert int(goff) == 0  # capture runs nothing
    for i in range(4):
        g.replay()
        assert torch.equal(out, eager[i]), i
    assert int(goff) == 4


@torch.no_grad()
def test_generate_with_in_graph_sampling_is_reproducible():
    from dlrover_wuqiong_amd.atorch.rl.hybrid_engine import HybridEngine
    from dlrover_wuqiong_amd.models.llama import Llama, LlamaConfig

    torch.manual_seed(0)
    cfg = LlamaConfig.named("llama-tiny")
    with torch.device(DEV):
        m = Llama(cfg)
    m = m.to(torch.bfloat16).eval()
    P, T = 7, 12
    p = torch.randint(0, cfg.vocab_size, (4, P), device=DEV)
    eng = HybridEngine(m, 4, 40, use_graph=True)
    a = eng.generate(p, T, temperature=1.0, top_p=0.9, fused_sampling=True, seed=1)
    assert int(eng.cache.lens[0]) == P + T - 1
    b = eng.generate(p, T, temperature=1.0, top_p=0.9, fused_sampling=True, seed=1)
    assert a.shape == (4, P + T) and torch.equal(a, b)
    assert torch.equal(a[:, :P], p) and int(a.min()) >= 0 and int(a.max()) < cfg.vocab_size
    assert int(eng.cache.lens[0]) == P + T - 1
    # the graph only changes how the step is launched
    eager = HybridEngine(m, 4, 40, use_graph=False).generate(p, T, temperature=1.0, top_p=0.9,
                                                             fused_sampling=True, seed=1)
    assert eager.shape == a.shape and int(eager.min()) >= 0 and int(eager.max()) < cfg.vocab_size
    assert not torch.equal(a, eng.generate(p, T, temperature=1.0, top_p=0.9, fused_sampling=True, seed=2))
