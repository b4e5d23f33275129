"""CPU mirror of the LDS-DMA staging of csrc/wgrad.hip (GLDS = true).

Three maps, written the way the kernel writes them:

* ``off(row, ch)``: byte offset of 16 B chunk ``ch`` of k-row ``row`` in
  one ``[64 k][128 columns]`` bf16 image (``lds_off_tr`` in mfma_tile.h);
* ``fill(tile, wave, t, lane)``: what the ``t``-th DMA wave-instruction
  of ``wave`` makes ``lane`` fetch, and the LDS byte it lands on;
* ``tr_addr(tile, wave, operand, frag, kh, h, lane)``: the LDS byte that
  ``lane`` supplies to the ``h``-th transposed read of one MFMA operand.

The constants are a copy of the kernel's; ``_C.wgrad_glds_layout()``
reports the kernel's own and test_wgrad_glds_gpu.py compares the two.
All LDS addresses are relative to one of the two buffers.
"""

BK = 64                 # k-rows of an image = the kernel's k-step
IMG_COLS = 128
IMG_BYTES = BK * IMG_COLS * 2
FILL_ROWS = 4           # image rows per DMA wave-instruction (1 KB)
FILLS_PER_WAVE = 8
BUFFERS = 2

# what _C.wgrad_glds_layout() must report beside "off" and "glds_default"
LAYOUT = {"bk": BK, "img_cols": IMG_COLS, "img_bytes": IMG_BYTES,
          "fill_rows": FILL_ROWS, "fills_per_wave": FILLS_PER_WAVE,
          "buffers": BUFFERS}

DY, X = 0, 1


def swz(row):
    return ((row & 3) << 2) | ((row >> 2) & 3)


def off(row, ch):
    return 256 * row + 16 * (ch ^ swz(row))


def off_table():
    return [off(row, ch) for row in range(BK) for ch in range(16)]


def images(tile):
    return tile // IMG_COLS


def operand_bytes(tile):
    return images(tile) * IMG_BYTES


def buffer_bytes(tile):
    return 2 * operand_bytes(tile)


def waves(tile):
    return tile // 32


def fill(tile, wave, t, lane):
    """-> (operand, k_row, tile_chunk, lds_byte): the lane fetches the
    16 B chunk ``tile_chunk`` (in units of 8 columns from the tile's first
    column, before the clamp) of k-row ``k_row`` of ``operand`` and the
    hardware puts it at ``lds_byte`` = wave-uniform base + 16 * lane."""
    wpo = tile // 64                        # filling waves per operand
    operand = wave // wpo
    grp = (wave % wpo) * FILLS_PER_WAVE     # first 4-row group of the wave
    img = grp // 16
    r0 = (grp % 16) * FILL_ROWS
    row = r0 + FILL_ROWS * t + (lane >> 4)
    ch = (lane & 15) ^ swz(row)
    base = (operand * operand_bytes(tile) + img * IMG_BYTES + r0 * 256 +
            t * FILL_ROWS * 256)
    return operand, row, img * 16 + ch, base + 16 * lane


def clamp_chunk(first_col, tile_chunk, ld):
    """Global 8-column chunk a fill really fetches in a row of ``ld``
    columns, for a tile that begins at column ``first_col``."""
    return min(first_col // 8 + tile_chunk, ld // 8 - 1)


def wave_origin(tile, wave):
    """(first dy column, first x column) of the wave's output quadrant."""
    return (wave >> 1) * 64, (wave & 1) * (tile // 2)


def frags(tile, operand):
    return 4 if operand == DY else tile // 32


def tr_addr(tile, wave, operand, frag, kh, h, lane):
    """LDS byte supplied by ``lane`` to transposed read ``h`` (0, 1) of
    fragment ``frag`` of ``operand`` in k-half ``kh``."""
    g, q, p = lane >> 4, (lane >> 2) & 3, lane & 3
    row = 8 * g + 4 * h + q
    o = off(row, p >> 1) + 8 * (p & 1)
    w0 = wave_origin(tile, wave)[operand]
    base = (o ^ (((w0 & 127) >> 4) << 5)) + (w0 >> 7) * IMG_BYTES
    if operand == X:
        base += operand_bytes(tile)
    return (base ^ (frag << 5)) + kh * 32 * 256


def bank(addr):
    return (addr // 4) % 64
