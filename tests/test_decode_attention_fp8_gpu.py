"""GPU: the MFMA split-KV decode kernel over an e4m3 KV cache
(``attn_decode_q8_kernel``, ``csrc/kernels/attn_decode.hip``) against softmax
attention in fp64 on the dequantised values ``codes.double() * scale.double()``.

Bound (from the reference alone): per (batch, head) row the L2 error is at most
``2 floor + ||slack||``: ``floor`` is the error of rounding the fp64 result to
bf16 (the factor 2 covers fp32 accumulation and the hardware ``exp2``, as in
``test_decode_attention_gpu.py``), and ``slack_d = 2^-9 sum_k p_k |v_kd|`` is
the hard bound on rounding each ``p v_scale`` once to bf16, the kernel's MFMA
operand.  K and the scores add nothing: e4m3 -> bf16 is exact and q stays bf16.

Caches and scales are strided views of larger buffers; everything outside the
valid keys of the right heads is poison: code 0x7F (e4m3 NaN) and NaN scales,
beyond Smax as well.  K/V are ``randn`` quantised by the cache's rule with the
quotients taken on the CPU (torch's GPU division is one ulp low now and then)."""

import math

import pytest
import torch

from dlrover_wuqiong_amd.ops.attention import decode_attention

pytestmark = pytest.mark.gpu
DEV = "cuda"
B = 3
FP8 = torch.float8_e4m3fn


def _cache(Smax, HKV, D, lens, seed):
    """codes [B, Smax, HKV, D] and scale [B, HKV, Smax]: views of poisoned
    [B, Smax + 9, 2 HKV, D] / [B, 2 HKV, Smax + 12] buffers."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, Smax, HKV, D, generator=g).to(torch.bfloat16).float()
    amax = x.abs().amax(-1)
    sc = torch.where(amax > 0, amax / 448.0, torch.ones_like(amax))
    codes = (x / sc[..., None]).clamp(-448, 448).to(FP8).view(torch.uint8)
    big = torch.full((B, Smax + 9, 2 * HKV, D), 0x7F, dtype=torch.uint8)
    bsc = torch.full((B, 2 * HKV, Smax + 12), float("nan"))
    for b, n in enumerate(lens):
        big[b, :n, :HKV] = codes[b, :n]
        bsc[b, :HKV, :n] = sc[b, :n].t()
    c, s = big.to(DEV).view(FP8)[:, :Smax, :HKV], bsc.to(DEV)[:, :HKV, :Smax]
    assert not c.is_contiguous() and not s.is_contiguous()
    return c, s


def _run(H, HKV, D, Smax, chunk, lens, seed, qmul=1.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    q = (qmul * torch.randn(B, H, D, device=DEV, generator=g)).to(torch.bfloat16)
    (kc, ks), (vc, vs) = _cache(Smax, HKV, D, lens, seed + 1), _cache(Smax, HKV, D, lens, seed + 2)
    out = decode_attention(q, kc, vc, torch.tensor(lens, device=DEV, dtype=torch.int32), chunk=chunk, k_scale=ks,
                           v_scale=vs)
    assert out.dtype == torch.bfloat16 and out.shape == q.shape
    assert bool(torch.isfinite(out).all()), "a key outside [0, len) reached the output"
    G = H // HKV
    for b, n in enumerate(lens):
        if n == 0:
            assert bool((out[b] == 0).all()), "len = 0 must give exact zeros"
            continue
        k = (kc[b, :n].double() * ks[b, :, :n].double().t()[..., None]).repeat_interleave(G, dim=1)  # [n, H, D]
        v = (vc[b, :n].double() * vs[b, :, :n].double().t()[..., None]).repeat_interleave(G, dim=1)
        p = (torch.einsum("hd,nhd->hn", q[b].double(), k) / math.sqrt(D)).softmax(-1)
        ref = torch.einsum("hn,nhd->hd", p, v)
        slack = 2.0 ** -9 * torch.einsum("hn,nhd->hd", p, v.abs())
        err = (out[b].double() - ref).norm(dim=-1)
        bound = 2 * (ref.to(torch.bfloat16).double() - ref).norm(dim=-1) + slack.norm(dim=-1)
        print(f"[decode fp8 D={D} H={H}/{HKV} Smax={Smax} lens={lens} b={b}] max err / bound = "
              f"{float((err / bound).max()):.4f}")
        assert bool((err <= bound).all()), float((err / bound).max())


# chunk boundaries; 32-key tile boundaries; an empty row; a cache shorter than a chunk
LENGTHS = [(600, 256, (600, 1, 333)), (600, 256, (256, 257, 255)), (600, 256, (0, 512, 513)),
           (200, 64, (31, 32, 33)), (40, 256, (40, 1, 17))]
# G = 1, 4, a partial tile, a full 16-row tile, a second head group of one
HEADS = [(8, 8), (8, 2), (6, 2), (16, 1), (17, 1)]


@pytest.mark.parametrize("Smax,chunk,lens", LENGTHS)
@pytest.mark.parametrize("H,HKV", HEADS)
@pytest.mark.parametrize("D", [64, 128])
def test_decode_fp8_strided_poisoned_caches(D, H, HKV, Smax, chunk, lens):
    _run(H, HKV, D, Smax, chunk, lens, seed=D + H + Smax)


@pytest.mark.parametrize("D", [64, 128])
def test_decode_fp8_one_hot_softmax(D):
    _run(6, 2, D, 600, 256, (600, 258, 31), seed=6, qmul=12.0)
