"""Exact tests of the atomic scatter kernels' row-segment map.

``emb_bwd_sgd``, ``emb_bwd_dense`` and ``emb_bwd_sgd_fused_wide`` give one
lane one float of an update row (``scatter_row_segments`` in
embedding.hip).  Tables and gradients here are small integers and every
scale factor is a power of two, so each table entry is an exact fp32 sum
whatever order the atomics arrive in (see exact_ints.py): the float64
``index_add_`` reference must be reproduced bit for bit, and a lost,
doubled or misplaced add moves an integer sum and fails ``torch.equal``.

Each shape is the smallest that reaches one branch of the map or of its
launch arithmetic; the comment beside it names the branch.
"""

import pytest
import torch

import exact_ints
from tf_yarn_amd import ops

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")

F32, BF16 = torch.float32, torch.bfloat16
AMAX = 4          # |table|, |grad| <= 4: exact in bf16
LR, SCALE = 0.5, 1.0   # SGD entries: alpha = -0.5
DENSE_SCALE = 2.0      # emb_bwd_dense: alpha = +2

# launch arithmetic of launch_row_segments (embedding.hip): one element per
# thread per trip, 256 threads, at most 8192 blocks
ELEMS_PER_TRIP = 256 * 8192

# dims: 4..64 divide the wave; 12 does not (rows straddle waves); 128 is
# wider than a wave; 7 and 1 are no multiple of 4 (scalar gradient
# rows; the runtime-dim instantiation serves them too)
DIMS = (4, 8, 16, 32, 64, 12, 128, 7, 1)
# n * dim off the wave (1, 3), off the block (67), many blocks with a
# ragged last one (70001)
TAILS = (1, 3, 67, 70001)


def _entry_dims(dims):
    """(entry, dim) pairs; the fused entry takes dim % 4 == 0 only."""
    return [(e, d) for e in ("sgd", "dense", "fused") for d in dims
            if e != "fused" or d % 4 == 0]


def _assert_exact(n, alpha):
    """Worst case: every update lands on one entry."""
    assert AMAX * n * abs(alpha) + AMAX < exact_ints.EXACT_LIMIT


def _operands(n, dim, rows, seed, ids=None):
    gen = torch.Generator().manual_seed(seed)
    table = exact_ints.ints((rows, dim), AMAX, gen)
    grad = exact_ints.ints((n, dim), AMAX, gen)
    if ids is None:
        ids = torch.randint(0, rows, (n,), generator=gen)
    return table, grad, ids


def _ref(table, ids, grad, alpha):
    out = table.double().clone()
    out.index_add_(0, ids, grad.double().reshape(ids.numel(), -1),
                   alpha=alpha)
    return out.float()


def _run_single(entry, table, ids, grad, gdtype):
    """One of the two single-table entry points; returns (got, want)."""
    alpha = -LR * SCALE if entry == "sgd" else DENSE_SCALE
    _assert_exact(ids.numel(), alpha)
    t = table.to(F32).cuda()
    g = grad.to(gdtype).cuda()
    if entry == "sgd":
        ops.emb_bwd_sgd(t, ids.cuda(), g, lr=LR, scale=SCALE)
    else:
        ops.emb_bwd_dense(t, ids.cuda(), g, scale=DENSE_SCALE)
    return t.cpu(), _ref(table, ids, grad, alpha)


def _run_fused(table, wide, ids, grad, gw, gdtype):
    """Returns (deep got, deep want, wide got, wide want)."""
    alpha = -LR * SCALE
    _assert_exact(ids.numel(), alpha)
    g_div = ids.numel() // gw.numel()
    t, w = table.to(F32).cuda(), wide.to(F32).cuda()
    ops.emb_bwd_sgd_fused_wide(t, w, ids.cuda(), grad.to(gdtype).cuda(),
                               gw.to(gdtype).cuda(), lr=LR, scale=SCALE)
    want_w = _ref(wide, ids, gw.repeat_interleave(g_div).reshape(-1, 1),
                  alpha)
    return t.cpu(), _ref(table, ids, grad, alpha), w.cpu(), want_w


def _wide_operands(n, rows, g_div, seed):
    gen = torch.Generator().manual_seed(seed + 1000)
    return (exact_ints.ints((rows, 1), AMAX, gen),
            exact_ints.ints((n // g_div,), AMAX, gen))


@requires_gpu
@pytest.mark.parametrize("gdtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("n", TAILS)
@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("entry", ["sgd", "dense"])
def test_single_table_dims_and_tails(entry, dim, n, gdtype):
    rows = 1009  # few rows: at n = 70001 every row collects ~70 adds
    table, grad, ids = _operands(n, dim, rows, seed=dim * 7 + n)
    got, want = _run_single(entry, table, ids, grad, gdtype)
    assert torch.equal(got, want)


@requires_gpu
@pytest.mark.parametrize("gdtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("n", TAILS)
@pytest.mark.parametrize("dim", [d for d in DIMS if d % 4 == 0])
def test_fused_wide_dims_and_tails(dim, n, gdtype):
    rows = 1009
    table, grad, ids = _operands(n, dim, rows, seed=dim * 11 + n)
    wide, gw = _wide_operands(n, rows, 1, seed=dim + n)
    got, want, got_w, want_w = _run_fused(table, wide, ids, grad, gw,
                                          gdtype)
    assert torch.equal(got, want)
    assert torch.equal(got_w, want_w)


@requires_gpu
@pytest.mark.parametrize("gdtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("g_div", [1, 26])
@pytest.mark.parametrize("dim", [4, 16, 64])
def test_fused_wide_add_once_per_update(dim, g_div, gdtype):
    """The wide table takes exactly one add per update row: with all-ones
    wide gradients and lr * scale = 0.5 it drops by half the number of
    times each row was hit, whatever the deep dim."""
    rows, n = 211, 26 * 2693  # 70018 updates: several blocks, ragged
    table, grad, ids = _operands(n, dim, rows, seed=dim + g_div)
    wide = torch.zeros(rows, 1, dtype=torch.int16)
    gw = torch.ones(n // g_div, dtype=torch.int16)
    got, want, got_w, want_w = _run_fused(table, wide, ids, grad, gw,
                                          gdtype)
    assert torch.equal(got, want)
    hits = torch.bincount(ids, minlength=rows).float().reshape(rows, 1)
    assert torch.equal(want_w, -0.5 * hits)
    assert torch.equal(got_w, want_w)
    # and with random wide gradients, shared by g_div consecutive updates
    wide, gw = _wide_operands(n, rows, g_div, seed=dim)
    got, want, got_w, want_w = _run_fused(table, wide, ids, grad, gw,
                                          gdtype)
    assert torch.equal(got, want)
    assert torch.equal(got_w, want_w)


@requires_gpu
@pytest.mark.parametrize("entry", ["sgd", "dense", "fused"])
def test_grid_stride_wrap(entry):
    """More elements than one trip of the capped grid covers, by a ragged
    8929 rows: the first 8929 * 16 threads loop twice."""
    dim, rows = 16, 4001
    n = 140001
    assert n * dim > ELEMS_PER_TRIP
    table, grad, ids = _operands(n, dim, rows, seed=5)
    if entry == "fused":
        wide, gw = _wide_operands(n, rows, 1, seed=5)
        got, want, got_w, want_w = _run_fused(table, wide, ids, grad, gw,
                                              BF16)
        assert torch.equal(got_w, want_w)
    else:
        got, want = _run_single(entry, table, ids, grad, BF16)
    assert torch.equal(got, want)


@requires_gpu
@pytest.mark.parametrize("gdtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("hot_rows", [1, 8])
@pytest.mark.parametrize("dim", [4, 16, 12, 128])
@pytest.mark.parametrize("entry", ["sgd", "dense", "fused"])
def test_collisions(entry, dim, hot_rows, gdtype):
    """All 4099 updates into one row, or into 8 rows."""
    rows, n = 64, 4099
    gen = torch.Generator().manual_seed(hot_rows)
    hot = torch.randperm(rows, generator=gen)[:hot_rows]
    ids = hot[torch.randint(0, hot_rows, (n,), generator=gen)]
    table, grad, _ = _operands(n, dim, rows, seed=dim, ids=ids)
    if entry == "fused":
        wide, gw = _wide_operands(n, rows, 1, seed=dim)
        got, want, got_w, want_w = _run_fused(table, wide, ids, grad, gw,
                                              gdtype)
        assert torch.equal(got_w, want_w)
    else:
        got, want = _run_single(entry, table, ids, grad, gdtype)
    assert torch.equal(got, want)
    cold = torch.ones(rows, dtype=torch.bool)
    cold[hot] = False
    assert torch.equal(got[cold], table.float()[cold])


@requires_gpu
@pytest.mark.parametrize("entry,dim", _entry_dims([16, 12, 128, 7]))
def test_boundary_rows(entry, dim):
    """Only the first and the last row are updated; their neighbours and
    everything between stay as they were."""
    rows, n = 50, 67
    ids = torch.where(torch.arange(n) % 3 == 0, 0, rows - 1)
    table, grad, _ = _operands(n, dim, rows, seed=dim, ids=ids)
    if entry == "fused":
        wide, gw = _wide_operands(n, rows, 1, seed=dim)
        got, want, got_w, want_w = _run_fused(table, wide, ids, grad, gw,
                                              BF16)
        assert torch.equal(got_w, want_w)
        assert torch.equal(got_w[1:-1], wide.float()[1:-1])
    else:
        got, want = _run_single(entry, table, ids, grad, BF16)
    assert torch.equal(got, want)
    assert not torch.equal(got[0], table.float()[0])
    assert not torch.equal(got[-1], table.float()[-1])
    assert torch.equal(got[1:-1], table.float()[1:-1])


@requires_gpu
@pytest.mark.parametrize("gdtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("entry,dim",
                         _entry_dims([4, 16, 64, 12, 128, 7]))
def test_position_coded(entry, dim, gdtype):
    """Unique ids into a zero table, ``g[i, c] = code(i, c)``: every table
    entry names the one (update, column) it must have come from, which
    catches a permutation inside a row.  fp32 codes are unique over the
    whole gradient; bf16 holds integers up to 256 only, so its codes
    repeat every 255 but still differ between neighbouring columns and
    updates."""
    n, rows = 4099, 5003
    gen = torch.Generator().manual_seed(dim)
    ids = torch.randperm(rows, generator=gen)[:n]
    i = torch.arange(n).reshape(n, 1)
    c = torch.arange(dim).reshape(1, dim)
    if gdtype == F32:
        code = i * dim + c + 1
        assert code.max() * 2 < exact_ints.EXACT_LIMIT
    else:
        code = 1 + (c + 3 * i) % 255
    alpha = DENSE_SCALE if entry == "dense" else -LR * SCALE
    t = torch.zeros(rows, dim, device="cuda")
    g = code.to(gdtype).cuda()
    if entry == "sgd":
        ops.emb_bwd_sgd(t, ids.cuda(), g, lr=LR, scale=SCALE)
    elif entry == "dense":
        ops.emb_bwd_dense(t, ids.cuda(), g, scale=DENSE_SCALE)
    else:
        w = torch.zeros(rows, 1, device="cuda")
        gw = (1 + torch.arange(n) % 255).to(gdtype)
        ops.emb_bwd_sgd_fused_wide(t, w, ids.cuda(), g, gw.cuda(), lr=LR,
                                   scale=SCALE)
        want_w = torch.zeros(rows, 1)
        want_w[ids, 0] = alpha * gw.float()
        assert torch.equal(w.cpu(), want_w)
    want = torch.zeros(rows, dim)
    want[ids] = alpha * code.float()
    assert torch.equal(t.cpu(), want)


# (offset, row stride) of the gradient slice inside the wider buffer: the
# model's own layout (13 dense + 3 pad columns, then 26 * 16, nothing
# after), a slice that is the whole buffer (dense kernel path), and one
# with columns on both sides
STRIDED_LAYOUTS = [(16, 432), (0, 416), (16, 448)]


@requires_gpu
@pytest.mark.parametrize("gdtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("off,stride", STRIDED_LAYOUTS)
def test_fused_wide_strided_source(off, stride, gdtype):
    """A column slice of a wider row-major buffer, read in place, gives
    what the dense copy of that slice gives.  The columns outside the
    slice hold 64s: a read that strays there cannot go unnoticed."""
    B, F, dim, rows = 37, 26, 16, 509
    n = B * F
    table, grad, ids = _operands(n, dim, rows, seed=off + stride)
    wide, gw = _wide_operands(n, rows, F, seed=stride)
    buf = torch.full((B, stride), 64, dtype=torch.int16)
    buf[:, off:off + F * dim] = grad.reshape(B, F * dim)
    buf = buf.to(gdtype).cuda()
    view = buf[:, off:off + F * dim]
    assert view.is_contiguous() == (stride == F * dim)
    got, want, got_w, want_w = _run_fused(table, wide, ids, grad, gw,
                                          gdtype)
    t, w = table.to(F32).cuda(), wide.to(F32).cuda()
    ops.emb_bwd_sgd_fused_wide(t, w, ids.cuda(), view,
                               gw.to(gdtype).cuda(), lr=LR, scale=SCALE)
    assert torch.equal(t.cpu(), got) and torch.equal(w.cpu(), got_w)
    assert torch.equal(got, want) and torch.equal(got_w, want_w)
    assert torch.equal(buf[:, :off].cpu().float(),
                       torch.full((B, off), 64.0))


@requires_gpu
def test_fused_wide_strided_source_runtime_dim():
    """The same through the runtime-dim instantiation (dim 8), several
    blocks."""
    B, F, dim, rows, off, stride = 1031, 5, 8, 211, 4, 52
    n = B * F
    table, grad, ids = _operands(n, dim, rows, seed=8)
    wide, gw = _wide_operands(n, rows, F, seed=8)
    buf = torch.full((B, stride), 64, dtype=torch.int16)
    buf[:, off:off + F * dim] = grad.reshape(B, F * dim)
    view = buf.to(BF16).cuda()[:, off:off + F * dim]
    _, want, _, want_w = _run_fused(table, wide, ids, grad, gw, BF16)
    t, w = table.to(F32).cuda(), wide.to(F32).cuda()
    ops.emb_bwd_sgd_fused_wide(t, w, ids.cuda(), view, gw.to(BF16).cuda(),
                               lr=LR, scale=SCALE)
    assert torch.equal(t.cpu(), want) and torch.equal(w.cpu(), want_w)
