"""The LDS image of the wgrad kernels' LDS-DMA staging, checked on the CPU
over the Python mirror in wgrad_image.py: a wrong DMA source or
destination faults the GPU, a wrong fragment address silently feeds the
MFMAs the wrong operand, so every address is enumerated here first.

Hardware rules the checks model (LDS-DMA: the destination is a
wave-uniform base + 16 * lane, the source is per lane; transposed read:
lane 4q+p of a 16-lane group supplies 8 bytes = row q, columns
4p..4p+3 of a 4 x 16 block, lane i receives column i with row q in
element q; its banks are (a / 4) % 64, counted per 32-lane half).
"""

import pytest

import wgrad_image as wi
from tf_yarn_amd import ops

TILES = (128, 256)


def test_off_is_a_bijection_onto_the_image():
    offs = wi.off_table()
    assert len(offs) == 64 * 16
    assert sorted(offs) == list(range(0, wi.IMG_BYTES, 16))


@pytest.mark.skipif(not ops.HAVE_EXT, reason="extension not built")
def test_mirror_matches_the_kernel_constants():
    lay = dict(ops._C.wgrad_glds_layout())
    assert list(lay.pop("off")) == wi.off_table()
    assert set(dict(lay.pop("glds_default"))) == set(TILES)
    assert lay == wi.LAYOUT


def _filled(tile):
    """LDS byte (16-aligned) -> (operand, k_row, tile_chunk) over all the
    fills of one k-step; asserts the per-instruction rules on the way."""
    image = {}
    for wave in range(wi.waves(tile)):
        for t in range(wi.FILLS_PER_WAVE):
            dst = [wi.fill(tile, wave, t, lane) for lane in range(64)]
            # one contiguous, 1 KB-aligned KB in lane order
            base = dst[0][3]
            assert base % 1024 == 0
            assert [d[3] for d in dst] == [base + 16 * l for l in range(64)]
            for op, row, ch, byte in dst:
                assert 0 <= row < wi.BK and 0 <= ch < tile // 8
                assert byte not in image
                image[byte] = (op, row, ch)
            # each 16-lane group reads one contiguous 256 B row segment
            for g in range(4):
                grp = dst[16 * g:16 * g + 16]
                assert len({(d[0], d[1]) for d in grp}) == 1
                chunks = sorted(d[2] for d in grp)
                assert chunks == list(range(chunks[0], chunks[0] + 16))
                assert chunks[0] % 16 == 0
    return image


@pytest.mark.parametrize("tile", TILES)
def test_fills_cover_one_buffer_exactly(tile):
    image = _filled(tile)
    assert sorted(image) == list(range(0, wi.buffer_bytes(tile), 16))
    assert 2 * wi.buffer_bytes(tile) == 4 * tile * 128  # the kernel's array
    want = {(op, row, ch) for op in (wi.DY, wi.X) for row in range(wi.BK)
            for ch in range(tile // 8)}
    assert set(image.values()) == want
    # a fill puts logical chunk ch of row `row` where off() says
    for byte, (op, row, ch) in image.items():
        assert byte == (op * wi.operand_bytes(tile) +
                        (ch // 16) * wi.IMG_BYTES + wi.off(row, ch % 16))


@pytest.mark.parametrize("tile", TILES)
def test_fragment_reads_see_the_mfma_operand(tile):
    """For every (wave, operand, fragment, kh, lane) the two transposed
    reads deliver [col = lane & 15][k = kh*32 + (lane >> 4)*8 + j]."""
    image = _filled(tile)
    for wave in range(wi.waves(tile)):
        for op in (wi.DY, wi.X):
            col0 = wi.wave_origin(tile, wave)[op]
            for frag in range(wi.frags(tile, op)):
                for kh in range(2):
                    addr = [[wi.tr_addr(tile, wave, op, frag, kh, h, lane)
                             for lane in range(64)] for h in range(2)]
                    for h in range(2):
                        for a in addr[h]:
                            assert a % 8 == 0
                            assert 0 <= a and a + 8 <= wi.buffer_bytes(tile)
                        # conflict-free: a half's 32 lanes x 2 banks differ
                        for half in (addr[h][:32], addr[h][32:]):
                            banks = [wi.bank(a + d) for a in half
                                     for d in (0, 4)]
                            assert len(set(banks)) == 64
                    for lane in range(64):
                        g, i = lane >> 4, lane & 15
                        for j in range(8):
                            h, q = j >> 2, j & 3
                            src = addr[h][16 * g + 4 * q + (i >> 2)]
                            byte = src + 2 * (i & 3)
                            got_op, row, ch = image[byte & ~15]
                            col = 8 * ch + (byte & 15) // 2
                            assert got_op == op
                            assert row == kh * 32 + g * 8 + j
                            assert col == col0 + frag * 16 + i


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("M", [8, 136, 264, 432])
def test_no_source_column_reaches_the_row_end(tile, M):
    for first_col in range(0, M, tile):
        for wave in range(wi.waves(tile)):
            for t in range(wi.FILLS_PER_WAVE):
                for lane in range(64):
                    op, row, ch, _ = wi.fill(tile, wave, t, lane)
                    if op != wi.X:
                        continue
                    gc = wi.clamp_chunk(first_col, ch, M)
                    assert 0 <= gc and 8 * gc + 8 <= M
                    # a chunk inside the row is fetched as itself
                    if first_col + 8 * ch + 8 <= M:
                        assert gc == first_col // 8 + ch


@pytest.mark.parametrize("tile", TILES)
def test_dy_never_clamps(tile):
    N = 2 * tile
    for first_col in (0, tile):
        for ch in range(tile // 8):
            assert wi.clamp_chunk(first_col, ch, N) == first_col // 8 + ch
