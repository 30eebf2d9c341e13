"""The LDS-DMA staging of the attention kernels (attn_fwd.hip / attn_bwd.hip):
a global_load_lds_dwordx4 writes LDS lane-linearly (1024 * chunk + 16 * lane),
so each lane fetches the global chunk that the T10(a) image (attn_common.h
img_off) places at its LDS position.  Pin, in Python, that the source-address
decode those kernels use (attn_common.h dma_rc) is the exact inverse of
img_off over a whole tile."""

import pytest


def img_off(D, row, ch):
    return (D * 16) * (row >> 3) + 512 * (ch >> 2) + 64 * (row & 7) + 16 * ((ch & 3) ^ ((row >> 2) & 3))


def dma_rc(D, ci, lane):  # mirrors dma_rc<D>() in attn_common.h
    halves = D // 64
    row = 8 * (ci // halves) + ((lane & 31) >> 2)
    ch = 4 * (2 * (ci % halves) + (lane >> 5)) + ((lane & 3) ^ ((row >> 2) & 3))
    return row, ch


# tile heights: the dK/dV query tiles (32 at D = 128, 64 at D = 64), the
# forward / dQ key tiles (64, 128) and the dK/dV block's V image (128)
@pytest.mark.parametrize("rows", [32, 64, 128])
@pytest.mark.parametrize("D", [64, 128])
def test_lds_dma_source_decode_inverts_img_off(D, rows):
    tile = rows * D * 2
    seen = set()
    for ci in range(tile // 1024):
        for lane in range(64):
            row, ch = dma_rc(D, ci, lane)
            assert 0 <= row < rows and 0 <= ch < D // 8
            assert img_off(D, row, ch) == 1024 * ci + 16 * lane
            seen.add((row, ch))
    assert len(seen) == rows * D // 8  # every 16-byte chunk of the tile exactly once
