"""GPU: the rollout kernels (``csrc/kernels/rollout.hip``) against the unfused
chain / the torch fallback, and the ragged hybrid engine: teacher-forced
logits against full forwards, fused K/V append against the unfused decode
step, graph replay against eager."""

import pytest
import torch

from dlrover_wuqiong_amd.atorch.rl.hybrid_engine import HybridEngine
from dlrover_wuqiong_amd.models.llama import Llama, LlamaConfig
from dlrover_wuqiong_amd.ops.rollout import kv_append_rope, rollout_step
from dlrover_wuqiong_amd.ops.rope import qkv_split_rope, rope_table

pytestmark = pytest.mark.gpu

B, SMAX = 3, 20


def _cache(NKV, D):
    """k / v caches [3, 20, NKV, D] cut out of a random [2, 4, 21, NKV, D]
    tensor: real batch / row strides, and a spare batch row and a spare
    sequence row that no write may touch."""
    store = torch.randn(2, 4, SMAX + 1, NKV, D, device="cuda", dtype=torch.bfloat16)
    return store, store[0, :B, :SMAX], store[1, :B, :SMAX]


def _inputs(NH, NKV, D, S):
    torch.manual_seed(0)
    qkv = torch.randn(B, S, NH + 2 * NKV, D, device="cuda", dtype=torch.bfloat16)
    cos, sin = rope_table(SMAX, D, 10000.0, "cuda")
    return qkv, cos, sin


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("NH,NKV", [(8, 8), (32, 8), (16, 1), (4, 2)])
def test_kv_append_rope_decode(D, NH, NKV):
    """Bitwise equality with ``qkv_split_rope`` + ``index_copy_`` held (the
    same fp32 expression on the same table, contracted alike)."""
    qkv, cos, sin = _inputs(NH, NKV, D, 1)
    store, kc, vc = _cache(NKV, D)
    want = store.clone()
    lens = torch.tensor([0, 19, 7], device="cuda", dtype=torch.int32)
    q = kv_append_rope(qkv, NH, NKV, cos, sin, kc, vc, lens)
    rq, rk, rv = qkv_split_rope(qkv, NH, NKV, cos, sin, pos_ids=lens.view(B, 1))
    idx = torch.arange(B, device="cuda") * (SMAX + 1) + lens.long()
    want[0].view(4 * (SMAX + 1), NKV, D).index_copy_(0, idx, rk.view(B, NKV, D))
    want[1].view(4 * (SMAX + 1), NKV, D).index_copy_(0, idx, rv.view(B, NKV, D))
    assert q.is_contiguous() and torch.equal(q, rq)
    assert torch.equal(store, want)


@pytest.mark.parametrize("D,NH,NKV", [(64, 4, 2), (128, 32, 8)])
def test_kv_append_rope_rows_at_the_end_of_the_cache_write_nothing(D, NH, NKV):
    qkv, cos, sin = _inputs(NH, NKV, D, 1)
    store, kc, vc = _cache(NKV, D)
    want = store.clone()
    lens = torch.tensor([SMAX, 3, SMAX], device="cuda", dtype=torch.int32)
    q = kv_append_rope(qkv, NH, NKV, cos, sin, kc, vc, lens)
    rq, rk, rv = qkv_split_rope(qkv, NH, NKV, cos, sin, pos_ids=lens.view(B, 1))
    want[0, 1, 3], want[1, 1, 3] = rk[1, 0], rv[1, 0]
    assert torch.equal(q, rq)  # q is still produced (table row clamped)
    assert torch.equal(store, want)


@pytest.mark.parametrize("D,NH,NKV", [(64, 4, 2), (128, 32, 8)])
def test_kv_append_rope_prefill(D, NH, NKV):
    S = 5
    qkv, cos, sin = _inputs(NH, NKV, D, S)
    store, kc, vc = _cache(NKV, D)
    want = store.clone()
    q = kv_append_rope(qkv, NH, NKV, cos, sin, kc, vc)
    rq, rk, rv = qkv_split_rope(qkv, NH, NKV, cos, sin)
    want[0, :B, :S], want[1, :B, :S] = rk, rv
    assert torch.equal(q, rq)
    assert torch.equal(store, want)


@pytest.mark.parametrize("Bn", [5, 300])
@pytest.mark.parametrize("eos", [7, None])
def test_rollout_step_matches_fallback(Bn, eos):
    g = torch.Generator().manual_seed(Bn)
    L = 12
    state = dict(
        sampled=torch.randint(5, 10, (Bn, 1), generator=g),               # eos = 7 hit by about a fifth
        lens=torch.randint(0, L + 2, (Bn,), generator=g).int(),           # some columns past the row
        finished=(torch.rand(Bn, generator=g) < 0.3).int(),
        resp_len=torch.randint(0, 5, (Bn,), generator=g).int(),
        seq=torch.randint(0, 100, (Bn, L), generator=g),
        tok_out=torch.zeros(Bn, 1, dtype=torch.long),
        n_active=torch.zeros(1, dtype=torch.int32))
    # every mix in the small batch too: row 0 hits eos now, row 1 is done, row 2 runs on
    state["sampled"][:3, 0] = torch.tensor([7, 7, 5])
    state["finished"][:3] = torch.tensor([0, 1, 0], dtype=torch.int32)
    cpu = {k: v.clone() for k, v in state.items()}
    gpu = {k: v.cuda() for k, v in state.items()}
    for _ in range(2):  # the second step starts from the first one's state
        rollout_step(eos_token_id=eos, pad_token_id=3, **cpu)
        rollout_step(eos_token_id=eos, pad_token_id=3, **gpu)
        for k in cpu:
            assert torch.equal(gpu[k].cpu(), cpu[k]), k
    assert int(cpu["n_active"]) == int((cpu["finished"] == 0).sum()) > 0
    assert eos is None or int(cpu["finished"].sum()) > int(state["finished"].sum())


def _model():
    torch.manual_seed(0)
    cfg = LlamaConfig.named("llama-tiny")
    with torch.device("cuda"):
        m = Llama(cfg)
    return m.to(torch.bfloat16).eval()


LENS = [5, 9, 1, 12]


@torch.no_grad()
def test_ragged_teacher_forced_logits_match_full_forward():
    m = _model()
    Pmax, T = max(LENS), 6
    lens = torch.tensor(LENS, device="cuda")
    ids = torch.randint(1, m.cfg.vocab_size, (4, Pmax + T), device="cuda")  # row b: its first len_b + T cells
    prompts = ids[:, :Pmax].clone()
    outs = []
    for fused in (False, True):
        eng = HybridEngine(m, 4, 64, use_graph=False, fused_kv_append=fused)
        eng._ensure_cache(4, prompts.device, torch.bfloat16)
        got = [eng._forward(prompts, prefill=True, last=lens - 1)]
        assert eng.cache.lens.tolist() == LENS
        for t in range(T):
            got.append(eng._forward(ids.gather(1, (lens + t).view(4, 1)), prefill=False).clone())
        outs.append(torch.stack(got))
        assert eng.cache.lens.tolist() == [n + T for n in LENS]
    for t in range(T + 1):
        for b, n in enumerate(LENS):
            full = m(ids[b:b + 1, :n + t])[0, -1]
            torch.testing.assert_close(outs[0][t, b].float(), full.float(), atol=5e-2, rtol=5e-2)
    # fused K/V append: the same bits as the unfused chain at this size (dw_rope and the fused kernel contract a
    # few lanes differently; a bf16 rounding that tells them apart is rare: docs/rl_ragged_rollouts.md)
    assert torch.equal(outs[0], outs[1])


@torch.no_grad()
def test_ragged_graph_replay_matches_eager():
    m = _model()
    Pmax, T, pad = max(LENS), 12, 0
    lens = torch.tensor(LENS, device="cuda")
    prompts = torch.randint(1, m.cfg.vocab_size, (4, Pmax), device="cuda")
    eager = HybridEngine(m, 4, 40, use_graph=False)
    free = eager.generate_ragged(prompts, lens, T, temperature=0)[0]
    eos = int(free[1, LENS[1] + 3])  # row 1 stops after its fourth token at the latest
    kw = dict(temperature=0, eos_token_id=eos, pad_token_id=pad, eos_check_interval=4)
    want, _, want_len = eager.generate_ragged(prompts, lens, T, **kw)
    assert int(want_len[1]) <= 4
    graph = HybridEngine(m, 4, 40, use_graph=True, fused_kv_append=True)
    seq, _, resp = graph.generate_ragged(prompts, lens, T, **kw)
    assert torch.equal(seq, want) and torch.equal(resp, want_len)
    # fused sampler inside the captured step: reproducible, finished rows stay pad
    kw = dict(temperature=1.0, top_k=50, top_p=0.95, fused_sampling=True, seed=11, eos_token_id=eos,
              pad_token_id=pad, eos_check_interval=4)
    a, _, la = graph.generate_ragged(prompts, lens, T, **kw)
    b, _, lb = graph.generate_ragged(prompts, lens, T, **kw)
    assert torch.equal(a, b) and torch.equal(la, lb)
    for s, rl in ((seq, resp), (a, la)):
        cols = torch.arange(Pmax + T, device="cuda")[None]
        end = (lens + rl)[:, None]
        assert (s[cols.expand_as(s) >= end] == pad).all()
        hit = rl < T
        assert (s.gather(1, end - 1)[hit] == eos).all()
