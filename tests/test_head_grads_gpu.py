"""Tests of the single-logit head's own gradients out of fused passes:

* ``head_relu_bwd_grads``: ``head_relu_bwd_db`` that also accumulates
  ``dw_head = dl^T . y`` and ``db_head = dl.sum()`` in the same pass over
  ``y`` and hands all three vectors to ONE reduce;
* ``col_reduce_dot_sum``: ``col_reduce_dot`` with ``db`` from the same
  pass;
* the two autograd nodes that use them, switches on against switches off.

``dz`` and ``dbias`` must be ``head_relu_bwd_db``'s to the bit on random
operands.  The new sums are checked with integer operands (exact_ints.py),
where every fp32 sum is exact in any order: ``torch.equal`` against
float64, no tolerance.  Shapes are the rows of the launch-arithmetic table
in docs/Kernels.md.
"""

import pytest
import torch

import exact_ints
from tf_yarn_amd import ops

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")

F32, BF16 = torch.float32, torch.bfloat16

# rows x cols -> branch of the launch arithmetic (elementwise.hip)
HEAD_SHAPES = [
    (32808, 256),  # 8 row slots per block, 1024 blocks: the row loop wraps;
                   # 8192 partial rows of 516 go to the tall reducer
    (37, 512),     # 4 slots, ragged last group; 12 partial rows of 1028
                   # must still be summed as head_relu_bwd_db sums 12 x 512
    (70, 1024),    # block = octs = 128, one slot; the split-K reducer
    (1, 8),        # one row, one oct, 255 idle slots
    (50, 432),     # 54 octs do not divide 256: the separate pieces
]
HEAD_IDS = [f"{r}x{c}" for r, c in HEAD_SHAPES]


def _C():
    import tf_yarn_amd.ops._C as C
    return C


def _stored(out, ref64, out_bf16):
    want = exact_ints.rne_bf16(ref64) if out_bf16 else ref64.float()
    assert out.dtype == (BF16 if out_bf16 else F32)
    assert out.shape == want.shape
    return torch.equal(out.cpu(), want)


# ---- head_relu_bwd_grads ----------------------------------------------------

@requires_gpu
@pytest.mark.parametrize("out_bf16", [False, True])
@pytest.mark.parametrize("rows,cols", HEAD_SHAPES, ids=HEAD_IDS)
def test_dz_dbias_are_the_plain_head_kernels(rows, cols, out_bf16):
    """Random bf16 operands: nearly every product rounds and the fp32
    column sums depend on their order."""
    gen = torch.Generator().manual_seed(rows + cols)
    dl = torch.randn(rows, generator=gen).to(BF16).cuda()
    w = (torch.randn(cols, generator=gen) * 0.1).to(BF16).cuda()
    y = torch.relu(torch.randn(rows, cols, generator=gen)).to(BF16).cuda()
    want_dz, want_db = _C().head_relu_bwd_db(dl, w, y, out_bf16)
    dz, dbias, dw_head, db_head = _C().head_relu_bwd_grads(dl, w, y,
                                                           out_bf16)
    assert torch.equal(dz, want_dz)
    assert dbias.dtype == want_db.dtype and torch.equal(dbias, want_db)
    assert dw_head.shape == (cols,) and db_head.shape == (1,)
    if out_bf16:  # the Python op is the same call
        op = ops.head_relu_bwd_grads(dl, w, y)
        for got, want in zip(op, (dz, dbias, dw_head, db_head)):
            assert torch.equal(got, want)


@requires_gpu
@pytest.mark.parametrize("out_bf16", [False, True])
@pytest.mark.parametrize("rows,cols", HEAD_SHAPES, ids=HEAD_IDS)
def test_head_grads_exact(rows, cols, out_bf16):
    """Integer dl, w and y (y >= 0, about a third of it zero)."""
    exact_ints.assert_exact(2, 3, rows)
    gen = torch.Generator().manual_seed(rows * 3 + cols)
    dl = exact_ints.ints((rows,), 2, gen)
    w = exact_ints.ints((cols,), 2, gen)
    y = (exact_ints.ints((rows, cols), 3, gen) - 1 +
         exact_ints.ints((rows, cols), 1, gen)).clamp(min=0)
    y[0, 0], y[0, -1] = 0, 2
    assert (y == 0).any() and (y > 0).any() and y.max() <= 3
    dz, dbias, dw_head, db_head = _C().head_relu_bwd_grads(
        dl.to(BF16).cuda(), w.to(BF16).cuda(), y.to(BF16).cuda(), out_bf16)
    ref_dz = (dl.double().unsqueeze(1) * w.double().unsqueeze(0)) * (y > 0)
    assert torch.equal(dz.double().cpu(), ref_dz)
    assert _stored(dbias, ref_dz.sum(0), out_bf16)
    assert _stored(dw_head, dl.double() @ y.double(), out_bf16)
    assert _stored(db_head, dl.double().sum().reshape(1), out_bf16)


@requires_gpu
@pytest.mark.parametrize("rows,cols", HEAD_SHAPES, ids=HEAD_IDS)
def test_position_coded_y_names_its_row(rows, cols):
    """y[b, m] = 1 only at b = (41 * m) % rows, dl[b] = (b % 251) + 1:
    dw_head[m] is the code of that one row."""
    m = torch.arange(cols)
    b0 = (41 * m) % rows
    y = torch.zeros(rows, cols)
    y[b0, m] = 1.0
    dl = ((torch.arange(rows) % 251) + 1).float()
    w = torch.ones(cols)
    _, _, dw_head, db_head = _C().head_relu_bwd_grads(
        dl.to(BF16).cuda(), w.to(BF16).cuda(), y.to(BF16).cuda(), False)
    assert torch.equal(dw_head.cpu(), ((b0 % 251) + 1).float())
    assert torch.equal(db_head.cpu(), dl.double().sum().float().reshape(1))


# ---- col_reduce_dot_sum -----------------------------------------------------

@requires_gpu
@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("rows,cols", [
    (37, 432),          # the exact cases of col_reduce_dot: 1D map
    (21, 1028),         # the k > 0 loop
    (8192 + 5, 1028),   # the 1D map's grid wraps, with tail
    (10001, 256),       # multi-slot map, rows % 4 != 0
    (9, 8192),          # last legal width
    (4100, 16),         # 64 slots per block, 17 blocks, ragged last one
    (65536, 16),        # the wide-dense head: 256 blocks where 32 ran
])
def test_col_reduce_dot_sum_exact(rows, cols, dtype):
    x, dy = exact_ints.operands((rows, cols), (rows,), rows,
                                seed=rows + cols)
    xd, dyd = x.to(dtype).cuda(), dy.to(dtype).cuda()
    ref_dw = (x.double() * dy.double().unsqueeze(1)).sum(0)
    ref_db = dy.double().sum().reshape(1)
    plain = _C().col_reduce_dot(xd, dyd)
    assert plain.dtype == F32 and torch.equal(plain.cpu(), ref_dw.float())
    for out_bf16 in (False, True):
        dw, db = _C().col_reduce_dot_sum(xd, dyd, out_bf16)
        assert _stored(dw, ref_dw, out_bf16)
        assert _stored(db, ref_db, out_bf16)
        if not out_bf16:
            assert torch.equal(dw, plain)
    op_dw, op_db = ops.col_reduce_dot_sum(xd, dyd, BF16)
    assert _stored(op_dw, ref_dw, True) and _stored(op_db, ref_db, True)


# ---- autograd: switches on against switches off -----------------------------

_SWITCHES = ("MIYARN_TALL_REDUCE", "MIYARN_FUSED_HEAD_GRADS")
_B = 4160  # 65 k-steps of the custom wgrad; 130 partial rows at 256 columns


def _head_fn_grads():
    """LinearBiasReLUHeadFn at 4160 x 64 -> 256 -> 1.  |z| <= 2*64 + 2, so y
    is an integer bf16 holds, and every gradient is an exact integer sum
    (worst: dw_head, 2 * 130 * 4160 < 2^24)."""
    exact_ints.assert_exact(2, 130, _B)
    gen = torch.Generator().manual_seed(4160)
    x = exact_ints.ints((_B, 64), 2, gen)
    wt = exact_ints.ints((256, 64), 1, gen)
    bias = exact_ints.ints((256,), 2, gen)
    w_head = exact_ints.ints((256,), 1, gen)
    b_head = exact_ints.ints((1,), 2, gen)
    dl = exact_ints.ints((_B,), 2, gen)
    leaves = [t.to(BF16).cuda().requires_grad_()
              for t in (x, wt, bias, w_head, b_head)]
    out = ops.linear_bias_relu_head(*leaves)
    out.backward(dl.to(BF16).cuda())
    return [t.grad for t in leaves]


def _scalar_head_grads():
    """ScalarHeadFn at 4160 x 16, the wide-dense head's shape."""
    gen = torch.Generator().manual_seed(16)
    x = exact_ints.ints((_B, 16), 2, gen)
    w = exact_ints.ints((16,), 2, gen)
    b = exact_ints.ints((1,), 2, gen)
    dl = exact_ints.ints((_B,), 2, gen)
    leaves = [t.to(BF16).cuda().requires_grad_() for t in (x, w, b)]
    out = ops.ScalarHeadFn.apply(*leaves)
    out.backward(dl.to(BF16).cuda())
    ref_dw = dl.double() @ x.double()
    assert torch.equal(leaves[1].grad.cpu(), exact_ints.rne_bf16(ref_dw))
    assert torch.equal(leaves[2].grad.cpu(),
                       exact_ints.rne_bf16(dl.double().sum().reshape(1)))
    return [t.grad for t in leaves]


@requires_gpu
@pytest.mark.parametrize("run", [_head_fn_grads, _scalar_head_grads],
                         ids=["linear_bias_relu_head", "ScalarHeadFn"])
def test_autograd_switches_on_equals_off(run, monkeypatch):
    for name in _SWITCHES:
        monkeypatch.setenv(name, "1")
    on = run()
    for name in _SWITCHES:
        monkeypatch.setenv(name, "0")
    off = run()
    assert len(on) == len(off)
    for a, b in zip(on, off):
        assert a is not None and a.dtype == b.dtype and a.shape == b.shape
        assert torch.equal(a, b)
