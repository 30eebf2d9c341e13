"""GPU: the MFMA pass 1 over a bf16 KV cache (``attn_decode_mfma_kernel``,
``csrc/kernels/attn_decode.hip``, ``decode_attention(kernel="mfma")``) against
softmax attention in fp64 on the bf16 values.

Bound (from the reference alone): per (batch, head) row the L2 error is at most
``2 floor + ||slack||``: ``floor`` is the error of rounding the fp64 result to
bf16 (the factor 2 covers fp32 accumulation and the hardware ``exp2``, as in
``test_decode_attention_gpu.py``), and ``slack_d = 2^-9 sum_k p_k |v_kd|`` is
the hard bound on rounding each ``p`` once to bf16, the kernel's MFMA operand.
K and the scores add nothing: bf16 x bf16 products are exact in fp32.

Caches are strided views of larger buffers; everything outside the valid keys
of the right heads is bf16 NaN, beyond Smax as well."""

import math

import pytest
import torch

from dlrover_wuqiong_amd.atorch.rl.hybrid_engine import HybridEngine
from dlrover_wuqiong_amd.models.llama import Llama, LlamaConfig
from dlrover_wuqiong_amd.ops._hip import HipKernelError
from dlrover_wuqiong_amd.ops.attention import decode_attention

pytestmark = pytest.mark.gpu
DEV = "cuda"
B = 3


def _cache(Smax, HKV, D, lens, seed):
    """bf16 [B, Smax, HKV, D]: a view of a NaN-filled [B, Smax + 9, 2 HKV, D] buffer."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, Smax, HKV, D, generator=g).to(torch.bfloat16)
    big = torch.full((B, Smax + 9, 2 * HKV, D), float("nan"), dtype=torch.bfloat16)
    for b, n in enumerate(lens):
        big[b, :n, :HKV] = x[b, :n]
    c = big.to(DEV)[:, :Smax, :HKV]
    assert not c.is_contiguous()
    return c


def _run(H, HKV, D, Smax, chunk, lens, seed, qmul=1.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    q = (qmul * torch.randn(B, H, D, device=DEV, generator=g)).to(torch.bfloat16)
    kc, vc = _cache(Smax, HKV, D, lens, seed + 1), _cache(Smax, HKV, D, lens, seed + 2)
    out = decode_attention(q, kc, vc, torch.tensor(lens, device=DEV, dtype=torch.int32), chunk=chunk, kernel="mfma")
    assert out.dtype == torch.bfloat16 and out.shape == q.shape
    assert bool(torch.isfinite(out).all()), "a key outside [0, len) reached the output"
    G = H // HKV
    for b, n in enumerate(lens):
        if n == 0:
            assert bool((out[b] == 0).all()), "len = 0 must give exact zeros"
            continue
        k = kc[b, :n].double().repeat_interleave(G, dim=1)  # [n, H, D]
        v = vc[b, :n].double().repeat_interleave(G, dim=1)
        p = (torch.einsum("hd,nhd->hn", q[b].double(), k) / math.sqrt(D)).softmax(-1)
        ref = torch.einsum("hn,nhd->hd", p, v)
        slack = 2.0 ** -9 * torch.einsum("hn,nhd->hd", p, v.abs())
        err = (out[b].double() - ref).norm(dim=-1)
        bound = 2 * (ref.to(torch.bfloat16).double() - ref).norm(dim=-1) + slack.norm(dim=-1)
        print(f"[decode mfma D={D} H={H}/{HKV} Smax={Smax} lens={lens} b={b}] max err / bound = "
              f"{float((err / bound).max()):.4f}")
        assert bool((err <= bound).all()), float((err / bound).max())


# chunk boundaries; 32-key tile boundaries; an empty row; a cache shorter than a chunk
LENGTHS = [(600, 256, (600, 1, 333)), (600, 256, (256, 257, 255)), (600, 256, (0, 512, 513)),
           (200, 64, (31, 32, 33)), (40, 256, (40, 1, 17))]
# G = 1, 4, a partial tile, a full 16-column tile, a second head group of one
HEADS = [(8, 8), (8, 2), (6, 2), (16, 1), (17, 1)]


@pytest.mark.parametrize("Smax,chunk,lens", LENGTHS)
@pytest.mark.parametrize("H,HKV", HEADS)
@pytest.mark.parametrize("D", [64, 128])
def test_decode_mfma_strided_poisoned_caches(D, H, HKV, Smax, chunk, lens):
    _run(H, HKV, D, Smax, chunk, lens, seed=D + H + Smax)


@pytest.mark.parametrize("D", [64, 128])
def test_decode_mfma_one_hot_softmax(D):
    _run(6, 2, D, 600, 256, (600, 258, 31), seed=6, qmul=12.0)


def test_decode_mfma_misaligned_q_is_a_contract_error():
    q = torch.zeros(3 * 8 * 64 + 1, device=DEV, dtype=torch.bfloat16)[1:].view(3, 8, 64)  # contiguous, 2-byte offset
    kc = torch.zeros(3, 40, 2, 64, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(HipKernelError, match="16-byte aligned"):
        decode_attention(q, kc, kc, torch.full((3,), 40, device=DEV, dtype=torch.int32), kernel="mfma")


@torch.no_grad()
@pytest.mark.parametrize("fused_kv_append", [False, True])
def test_engine_mfma_graph_equals_eager(fused_kv_append):
    torch.manual_seed(0)
    with torch.device(DEV):
        m = Llama(LlamaConfig.named("llama-tiny")).to(torch.bfloat16).eval()
    prompts = torch.randint(1, m.cfg.vocab_size, (3, 5), device=DEV)
    seqs = [HybridEngine(m, 3, 16, use_graph=graph, fused_kv_append=fused_kv_append,
                         decode_kernel="mfma").generate(prompts, 8, temperature=0.0) for graph in (False, True)]
    assert seqs[0].shape == (3, 13) and torch.equal(seqs[0], seqs[1])
