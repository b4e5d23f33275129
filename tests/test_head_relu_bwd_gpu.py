"""Bit-exact tests of ``head_relu_bwd_db``: the ReLU backward + dbias of
the last hidden layer, computed from the logit gradient ``dl [B]`` and the
head weight ``w [cols]`` instead of their materialised outer product.

The reference is what the model ran before:
``bias_relu_bwd_db(dl[:, None] * w[None, :], y)``.  The kernel forms
``bf16(float(dl) * float(w))`` itself - one round-to-nearest-even of an
exact fp32 product, like torch's bf16 multiply - and keeps the oct map,
the partial slab and the reduce of ``bias_relu_bwd_dbpart8_kernel``, so
``dz`` AND ``dbias`` must be ``torch.equal``.  Shapes are the oct-kernel
rows of the table in docs/Kernels.md.
"""

import pytest
import torch

from tf_yarn_amd import ops

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")

BF16 = torch.bfloat16

# rows x cols -> branch of the launch arithmetic (elementwise.hip)
SHAPES = [
    (32808, 256),  # 8 row slots per block, 1024 blocks: the row loop wraps
    (37, 512),     # 4 slots, ragged last group of 4 rows
    (70, 1024),    # block = octs = 128, one slot
    (70, 2048),    # block = 256 octs
    (1, 8),        # one row, one oct, 255 idle slots
    (50, 432),     # 54 octs do not divide 256: the two-step path
]


def _y(rows, cols, gen):
    """ReLU output with zeros, negatives and positives in every column (a
    true ReLU output has no negatives; the mask must not care)."""
    y = torch.randn(rows, cols, generator=gen)
    if rows >= 3:
        y[0] = 0.0
        y[1] = -y[1].abs() - 0.01
        y[2] = y[2].abs() + 0.01
    else:  # a single row: mix the three kinds along it
        y[:, 0::3] = 0.0
        y[:, 1::3] = -y[:, 1::3].abs() - 0.01
        y[:, 2::3] = y[:, 2::3].abs() + 0.01
    return y.to(BF16).cuda()


def _check(dl, w, y):
    import tf_yarn_amd.ops._C as C
    want_dz, want_db = C.bias_relu_bwd_db(
        (dl.unsqueeze(1) * w.unsqueeze(0)).contiguous(), y, True)
    got_dz, got_db = C.head_relu_bwd_db(dl, w, y, True)
    assert got_dz.dtype == BF16 and got_db.dtype == BF16
    assert torch.equal(got_dz, want_dz)
    assert torch.equal(got_db, want_db)
    # the Python op is the same call
    op_dz, op_db = ops.head_relu_bwd_db(dl, w, y)
    assert torch.equal(op_dz, want_dz)
    assert torch.equal(op_db, want_db)
    return got_dz


@requires_gpu
@pytest.mark.parametrize("rows,cols", SHAPES,
                         ids=[f"{r}x{c}" for r, c in SHAPES])
def test_matches_outer_product_path(rows, cols):
    """Random bf16 operands: nearly every product needs rounding."""
    gen = torch.Generator().manual_seed(rows + cols)
    dl = torch.randn(rows, generator=gen).to(BF16).cuda()
    w = (torch.randn(cols, generator=gen) * 0.1).to(BF16).cuda()
    y = _y(rows, cols, gen)
    exact = dl.float().unsqueeze(1) * w.float().unsqueeze(0)
    assert (exact.to(BF16).float() != exact).float().mean() > 0.5
    dz = _check(dl, w, y)
    assert dz.any()


@requires_gpu
def test_products_on_rounding_ties():
    """dl = +-1.5 * 2^a and w = +-(1 + k/128) * 2^c with k odd and below
    42: every product has exactly 9 significant bits, the last one set -
    halfway between two bf16 values, where only round-to-nearest-EVEN
    agrees with torch."""
    rows, cols = 70, 256
    gen = torch.Generator().manual_seed(9)
    sign = lambda n: torch.randint(0, 2, (n,), generator=gen) * 2.0 - 1.0
    pow2 = lambda n: torch.pow(
        2.0, torch.randint(-3, 4, (n,), generator=gen).float())
    dl = 1.5 * sign(rows) * pow2(rows)
    k = torch.randint(0, 21, (cols,), generator=gen).float() * 2 + 1
    w = (1.0 + k / 128.0) * sign(cols) * pow2(cols)
    assert torch.equal(dl.to(BF16).float(), dl)
    assert torch.equal(w.to(BF16).float(), w)
    prod = dl.unsqueeze(1) * w.unsqueeze(0)
    assert ((prod.view(torch.int32) & 0xFFFF) == 0x8000).all()
    _check(dl.to(BF16).cuda(), w.to(BF16).cuda(), _y(rows, cols, gen))
