"""GPU: shared-prefix decode attention (``dw_attn_decode_shared``,
``csrc/kernels/attn_decode.hip``, ``ops.attention.decode_attention_shared``)
against softmax attention in fp64 over each row's valid prefix and suffix keys.

Bound (from the reference alone, that of ``test_decode_attention_mfma_gpu.py``):
per (row, head) the L2 error is at most ``2 floor + ||slack||``, ``floor`` the
error of rounding the fp64 result to bf16 and ``slack_d = 2^-9 sum_k p_k |v_kd|``
the bound on rounding each ``p`` once to bf16; the split merge is fp32 and is
covered by the factor 2.  Largest err / bound seen on an MI355X: see
docs/rl_shared_prefix.md.

Caches are strided views of larger buffers; everything outside the valid keys
of the right heads is bf16 NaN, beyond Pmax / Ssuf as well."""

import math

import pytest
import torch

from dlrover_wuqiong_amd.atorch.rl.hybrid_engine import HybridEngine
from dlrover_wuqiong_amd.models.llama import Llama, LlamaConfig
from dlrover_wuqiong_amd.ops._hip import HipKernelError
from dlrover_wuqiong_amd.ops.attention import decode_attention_shared

pytestmark = pytest.mark.gpu
DEV = "cuda"
BP, SSUF = 2, 70
SUFFIX = (0, 1, 31, 32, 33, 70)


def _cache(rows, Smax, HKV, D, lens, seed):
    """bf16 [rows, Smax, HKV, D]: a view of a NaN-filled [rows, Smax + 9, 2 HKV, D] buffer."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, Smax, HKV, D, generator=g).to(torch.bfloat16)
    big = torch.full((rows, Smax + 9, 2 * HKV, D), float("nan"), dtype=torch.bfloat16)
    for b, n in enumerate(lens):
        big[b, :n, :HKV] = x[b, :n]
    c = big.to(DEV)[:, :Smax, :HKV]
    assert not c.is_contiguous()
    return c


def _run(n, H, HKV, D, Pmax, chunk, plens, seed, qmul=1.0):
    B, G = BP * n, H // HKV
    slens = [SUFFIX[b % len(SUFFIX)] for b in range(B)]
    g = torch.Generator(device=DEV).manual_seed(seed)
    q = (qmul * torch.randn(B, H, D, device=DEV, generator=g)).to(torch.bfloat16)
    kp, vp = _cache(BP, Pmax, HKV, D, plens, seed + 1), _cache(BP, Pmax, HKV, D, plens, seed + 2)
    ks, vs = _cache(B, SSUF, HKV, D, slens, seed + 3), _cache(B, SSUF, HKV, D, slens, seed + 4)
    out = decode_attention_shared(q, kp, vp, torch.tensor(plens, device=DEV, dtype=torch.int32), ks, vs,
                                  torch.tensor(slens, device=DEV, dtype=torch.int32), n, chunk=chunk)
    assert out.dtype == torch.bfloat16 and out.shape == q.shape
    assert bool(torch.isfinite(out).all()), "a key outside the valid prefix / suffix reached the output"
    worst = 0.0
    for b in range(B):
        a, s = plens[b // n], slens[b]
        if a + s == 0:
            assert bool((out[b] == 0).all()), "a row with no key must give exact zeros"
            continue
        k = torch.cat([kp[b // n, :a], ks[b, :s]]).double().repeat_interleave(G, dim=1)  # [a + s, H, D]
        v = torch.cat([vp[b // n, :a], vs[b, :s]]).double().repeat_interleave(G, dim=1)
        p = (torch.einsum("hd,nhd->hn", q[b].double(), k) / math.sqrt(D)).softmax(-1)
        ref = torch.einsum("hn,nhd->hd", p, v)
        slack = 2.0 ** -9 * torch.einsum("hn,nhd->hd", p, v.abs())
        err = (out[b].double() - ref).norm(dim=-1)
        bound = 2 * (ref.to(torch.bfloat16).double() - ref).norm(dim=-1) + slack.norm(dim=-1)
        worst = max(worst, float((err / bound).max()))
        assert bool((err <= bound).all()), (b, float((err / bound).max()))
    print(f"[decode shared D={D} n={n} H={H}/{HKV} Pmax={Pmax} prefix={plens}] max err / bound = {worst:.4f}")


# prefix: chunk and 32-key tile boundaries, an empty prefix (rows with suffix 0 then have no key), a short cache
PREFIX = [(600, 256, (600, 1)), (600, 256, (256, 257)), (600, 256, (0, 513)), (200, 64, (31, 33))]
# (n, H, Hkv): n = 1; exactly 16 columns; 18 (a sample straddles the tile edge); 36 (three column tiles); G > 16; 48;
# 85 columns: a second block of column tiles whose last tiles are empty
HEADS = [(1, 8, 2), (4, 8, 2), (6, 6, 2), (9, 8, 2), (2, 17, 1), (3, 16, 1), (5, 17, 1)]


@pytest.mark.parametrize("Pmax,chunk,plens", PREFIX)
@pytest.mark.parametrize("n,H,HKV", HEADS)
@pytest.mark.parametrize("D", [64, 128])
def test_shared_strided_poisoned_caches(D, n, H, HKV, Pmax, chunk, plens):
    _run(n, H, HKV, D, Pmax, chunk, plens, seed=D + H + Pmax + n)


@pytest.mark.parametrize("D", [64, 128])
def test_shared_one_hot_softmax(D):
    _run(6, 6, 2, D, 600, 256, (600, 258), seed=6, qmul=12.0)


def test_shared_batch_mismatch_is_a_contract_error():
    q = torch.zeros(5, 8, 64, device=DEV, dtype=torch.bfloat16)   # 5 rows != 2 prompts x 3 samples
    kp = torch.zeros(2, 40, 2, 64, device=DEV, dtype=torch.bfloat16)
    ks = torch.zeros(5, 8, 2, 64, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(HipKernelError, match="B = Bp \\* samples_per_prompt"):
        decode_attention_shared(q, kp, kp, torch.full((2,), 40, device=DEV, dtype=torch.int32), ks, ks,
                                torch.zeros(5, device=DEV, dtype=torch.int32), 3)


@torch.no_grad()
@pytest.mark.parametrize("ragged", [False, True])
def test_engine_shared_graph_equals_eager(ragged):
    torch.manual_seed(0)
    with torch.device(DEV):
        m = Llama(LlamaConfig.named("llama-tiny")).to(torch.bfloat16).eval()
    prompts = torch.randint(1, m.cfg.vocab_size, (2, 5), device=DEV)
    lens, outs = torch.tensor([5, 3]), []
    if ragged:   # a token the free rollout draws third in prompt 0's rows: they stop there
        free = HybridEngine(m, 6, 16, use_graph=False).generate_ragged(prompts, lens, 8, temperature=0.0,
                                                                       samples_per_prompt=3)
        eos = int(free[0][0, 7])
    for graph in (False, True):
        eng = HybridEngine(m, 6, 16, use_graph=graph)
        if ragged:
            outs.append(eng.generate_ragged(prompts, lens, 8, temperature=0.0, eos_token_id=eos,
                                            samples_per_prompt=3, eos_check_interval=2))
        else:
            outs.append((eng.generate(prompts, 8, temperature=0.0, samples_per_prompt=3),))
    assert outs[0][0].shape == (6, 13)
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    if ragged:
        assert int(outs[0][2].min()) < 8, "no row stopped at the EOS"
