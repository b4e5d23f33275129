"""Exact tests of the radix-binned scatter (csrc/binned_scatter.hip).

Tables and gradients are small integers and ``alpha = -lr * scale = -0.5``,
so every table entry is an exact fp32 sum in any order, whether an update
went through the LDS hash (``alpha * sum(g)``) or through global atomics
(``sum(alpha * g)``); see exact_ints.py.  The float64 ``index_add_``
reference must come back bit for bit: a lost, doubled or misplaced add, a
slot left non-zero for the block's next bin or a gradient read from the
neighbouring update moves an integer sum and fails ``torch.equal``.

Every case aims at one branch of the kernels, named in the comment beside
it, and asserts on the CPU (with tests/binned_cases.py) the precondition
that makes its ids reach that branch.  Every table is the leading slice of
a buffer ``TAIL`` rows longer whose tail must stay untouched, and the whole
table is compared, so a misplaced write shows.
"""

import math

import pytest
import torch

import binned_cases as bc
import exact_ints
from tf_yarn_amd import ops

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")

F32, BF16 = torch.float32, torch.bfloat16
both_gdtypes = pytest.mark.parametrize("gdtype", [F32, BF16],
                                       ids=["f32", "bf16"])
both_kinds = pytest.mark.parametrize("kind", ["deep", "scalar"])

AMAX = 4               # |table|, |grad| <= 4: exact in bf16
LR, SCALE = 0.5, 1.0
ALPHA = -LR * SCALE    # -0.5
DIM = 16               # the deep kernel is a dim-16 kernel
CAP = {"deep": bc.HASH_DEEP, "scalar": bc.HASH_SCALAR}
TAIL = 64              # rows behind the table that must stay as they were
SENTINEL = 77.0
WIDE_BITS = 14         # the widest region ops.pick_region_bits chooses


def _assert_exact(ids, gmax=AMAX, tmax=AMAX, launches=1):
    """Worst case: every update of the most-hit row carries ``gmax``.  The
    hash path sums the raw gradients in LDS before scaling them."""
    hits = int(torch.bincount(ids.reshape(-1)).max()) if ids.numel() else 0
    assert gmax * hits < exact_ints.EXACT_LIMIT
    assert (launches * gmax * hits * abs(ALPHA) + tmax
            < exact_ints.EXACT_LIMIT)


def _operands(kind, n, n_rows, seed, g_div=1):
    """(table, grad as the kernel takes it, grad per update [n, dim])."""
    gen = torch.Generator().manual_seed(seed)
    dim = DIM if kind == "deep" else 1
    table = exact_ints.ints((n_rows, dim), AMAX, gen)
    if kind == "deep":
        grad = exact_ints.ints((n, dim), AMAX, gen)
        return table, grad, grad
    assert n % g_div == 0
    grad = exact_ints.ints((n // g_div,), AMAX, gen)
    return table, grad, grad.repeat_interleave(g_div).reshape(n, 1)


def _ref(table, ids, per_update):
    out = table.double().clone()
    out.index_add_(0, ids.reshape(-1), per_update.double(), alpha=ALPHA)
    return out.float()


def _padded(table):
    """The table as the leading rows of a longer GPU buffer."""
    n_rows, dim = table.shape
    buf = torch.full((n_rows + TAIL, dim), SENTINEL)
    buf[:n_rows] = table.float()
    buf = buf.cuda()
    view = buf[:n_rows]
    assert view.is_contiguous() and view.data_ptr() == buf.data_ptr()
    return buf, view


def _launch(kind, view, ids, grad, bits=None, perm=None):
    if kind == "deep":
        ops.emb_bwd_sgd_binned(view, ids, grad, lr=LR, scale=SCALE,
                               perm=perm, region_bits=bits)
    else:
        ops.emb_scatter_sum_binned(view, ids, grad, alpha=ALPHA,
                                   perm=perm, region_bits=bits)


def _assert_table(buf, want, what=""):
    got = buf.cpu()
    n_rows = want.shape[0]
    bad = (got[:n_rows] != want).any(dim=1).nonzero().reshape(-1)
    assert torch.equal(got[:n_rows], want), (
        f"{what}: {bad.numel()} rows differ, first {bad[:8].tolist()}; "
        f"got {got[bad[0]].tolist()} want {want[bad[0]].tolist()}")
    assert torch.equal(got[n_rows:], torch.full_like(got[n_rows:],
                                                     SENTINEL)), \
        f"{what}: rows behind the table were written"


def _case(kind, ids, n_rows, bits, gdtype, seed, g_div=1):
    """One launch on integer operands against the float64 reference."""
    ids = ids.reshape(-1)
    _assert_exact(ids)
    table, grad, per_update = _operands(kind, ids.numel(), n_rows, seed,
                                        g_div)
    want = _ref(table, ids, per_update)
    if ids.numel() >= 16:  # the case must move something
        assert not torch.equal(want, table.float())
    buf, view = _padded(table)
    _launch(kind, view, ids.cuda(), grad.to(gdtype).cuda(), bits)
    _assert_table(buf, want, kind)


def _shuffled(ids, gen):
    return ids[torch.randperm(ids.numel(), generator=gen)]


def _repeat_1_to_5(keys, gen):
    """Each key 1 to 5 times, in random order."""
    reps = torch.randint(1, 6, (keys.numel(),), generator=gen)
    return _shuffled(keys.repeat_interleave(reps), gen)


@requires_gpu
def test_layout_matches_helper_constants():
    """Every case below is aimed with binned_cases' copy of the kernel's
    constants: a changed capacity, probe limit, threshold or multiplier
    must fail here, not quietly move the cases off their branches."""
    import tf_yarn_amd.ops._C as C
    assert dict(C.binned_layout()) == bc.LAYOUT
    for kind, cap in CAP.items():
        assert bc.LAYOUT[f"hash_max_count_{kind}"] == bc.hash_max_count(cap)


# ---- the use_hash switch -----------------------------------------------------

@requires_gpu
@both_gdtypes
@pytest.mark.parametrize("law", ["distinct", "one_row", "repeats"])
@pytest.mark.parametrize("edge", [-1, 0, 1])
@both_kinds
def test_hash_threshold(kind, edge, law, gdtype):
    """One bin of 767 / 768 / 769 (1535 / 1536 / 1537) updates: the last
    two counts the hash still takes, and the first that goes all-atomic.
    distinct: consecutive rows, so no two share a home (the bijection);
    one_row: one LDS slot takes every add; repeats: random rows."""
    cap = CAP[kind]
    count = bc.hash_max_count(cap) + edge
    n_rows, bits = cap, int(math.log2(cap))
    gen = torch.Generator().manual_seed(count)
    if law == "distinct":
        ids = _shuffled(5 + torch.arange(count), gen)
        assert bc.home(ids, cap).unique().numel() == count
    elif law == "one_row":
        ids = torch.full((count,), 37)
    else:
        ids = torch.randint(0, n_rows, (count,), generator=gen)
        assert 1 < ids.unique().numel() < count
    assert bc.bin_counts(ids, bits, n_rows).tolist() == [count]
    assert (count <= bc.hash_max_count(cap)) == (edge <= 0)
    _case(kind, ids, n_rows, bits, gdtype, seed=count)


@requires_gpu
@both_gdtypes
@both_kinds
def test_hot_row_inside_hash(kind, gdtype):
    """LDS float atomics on one slot: a bin of 768 (1536) updates of one
    row, the most the hash takes, and next to it a bin of 700 updates
    over 3 rows."""
    cap = CAP[kind]
    full = bc.hash_max_count(cap)
    bits, n_rows = 7, 256
    gen = torch.Generator().manual_seed(1)
    ids = _shuffled(torch.cat([
        torch.full((full,), 5),
        128 + torch.randint(0, 3, (700,), generator=gen)]), gen)
    assert bc.bin_counts(ids, bits, n_rows).tolist() == [full, 700]
    assert 700 <= full and ids.unique().numel() == 4
    _case(kind, ids, n_rows, bits, gdtype, seed=2)


# ---- the probe ---------------------------------------------------------------

@requires_gpu
@both_gdtypes
@both_kinds
def test_probe_wraps_at_capacity(kind, gdtype):
    """64 keys of bin 1 whose homes are the last 4 (8) slots: the cluster
    runs over ``capacity - 1 -> 0``.  With no more than PROBE_MAX keys in
    the bin none may give up (test_binned_cases.py), so every update goes
    through the hash and the plain writeback."""
    cap = CAP[kind]
    n_homes = 64 * cap // 2 ** WIDE_BITS  # a bin has 16 (8) rows per home
    homes = bc.consecutive_homes(cap - n_homes, n_homes, cap)
    keys = bc.rows_with_homes(1, WIDE_BITS, homes, cap)
    gen = torch.Generator().manual_seed(3)
    ids = _repeat_1_to_5(keys, gen)
    n_rows = 2 * 2 ** WIDE_BITS + 100
    assert keys.numel() == 64 <= bc.PROBE_MAX
    assert max(homes) == cap - 1 and keys.numel() > n_homes  # must wrap
    assert bc.bin_counts(ids, WIDE_BITS, n_rows).tolist() == \
        [0, ids.numel(), 0]
    assert ids.numel() <= bc.hash_max_count(cap)
    assert bc.simulate_probe(ids.tolist(), cap) == 0
    _case(kind, ids, n_rows, WIDE_BITS, gdtype, seed=4)


@requires_gpu
@both_gdtypes
@pytest.mark.parametrize("where", ["mid", "wrap"])
@both_kinds
def test_probe_gives_up(kind, where, gdtype):
    """128 keys of bin 1 on 8 (16) consecutive homes reach only 8 + 63
    (16 + 63) slots, so at least 57 (49) of them give up and go through
    global atomics, while the others and a few ordinary keys of the same
    bin go through the hash and the plain writeback.  Every thread that
    holds an update of one key must decide alike, or the row gets a plain
    write and an atomic at once."""
    cap = CAP[kind]
    n_homes, must = (8, 57) if kind == "deep" else (16, 49)
    first = cap // 2 if where == "mid" else cap - n_homes // 2
    crowded = bc.rows_with_homes(
        1, WIDE_BITS, bc.consecutive_homes(first, n_homes, cap), cap)
    far = bc.consecutive_homes(first + cap // 2, 5, cap)
    ordinary = torch.cat([bc.rows_with_homes(1, WIDE_BITS, [h], cap)[:1]
                          for h in far])
    gen = torch.Generator().manual_seed(5)
    ids = _repeat_1_to_5(torch.cat([crowded, ordinary]), gen)
    n_rows = 2 * 2 ** WIDE_BITS + 100
    assert crowded.numel() == 128 and ordinary.numel() == 5
    assert bc.min_give_ups(crowded.numel(), n_homes) == must
    # the ordinary keys sit out of the crowd's reach and of each other's way
    for h in far:
        assert (h - first) % cap > n_homes + bc.PROBE_MAX
        assert (first - h) % cap > len(far) + bc.PROBE_MAX
    assert bc.bin_counts(ids, WIDE_BITS, n_rows).tolist() == \
        [0, ids.numel(), 0]
    assert ids.numel() <= bc.hash_max_count(cap)  # the bin is hashed
    gave_up = bc.simulate_probe(ids.tolist(), cap)
    assert must <= gave_up < crowded.numel()
    _case(kind, ids, n_rows, WIDE_BITS, gdtype, seed=6)


# ---- many bins per block -------------------------------------------------------

MANY_BINS = 2 * bc.APPLY_GRID_MAX + 38   # 16422
HEAVY_BLOCKS = (0, 5, 17, 36)            # blocks that serve three bins
HEAVY_COUNT = {"deep": 800, "scalar": 1600}


def _many_bins_ids():
    gen = torch.Generator().manual_seed(7)
    per_bin = torch.randint(1, 4, (MANY_BINS,), generator=gen)
    per_bin[torch.rand(MANY_BINS, generator=gen) < 0.1] = 0
    per_bin[-1] = 1
    return gen, per_bin


@requires_gpu
@both_gdtypes
@both_kinds
def test_many_bins_per_block(kind, gdtype):
    """16422 two-row bins on 8192 blocks: blocks grid-stride over bins, so
    a block's next bin sees what the lazy reset left; empty bins are
    skipped; blocks 0, 5, 17 and 36 serve a hashed bin, then an
    all-atomic one (800 / 1600 updates), then a hashed one whose rows
    have the SAME home slots as the first bin's; the scan walks 17 bins
    per thread; the last bin holds one row.  A stale ``h_val`` shows here;
    a stale ``h_id`` whose ``h_val`` was cleared does not, and cannot in
    any test of results: it adds 0 to the old row and moves the new key
    one slot on."""
    cap = CAP[kind]
    bits = 1
    n_rows = 2 * (MANY_BINS - 1) + 1
    gen, per_bin = _many_bins_ids()
    stride = bc.APPLY_GRID_MAX
    for b in HEAVY_BLOCKS:
        per_bin[b] = 2
        per_bin[b + stride] = HEAVY_COUNT[kind]
        per_bin[b + 2 * stride] = 3
    bins = torch.arange(MANY_BINS).repeat_interleave(per_bin)
    rows = 2 * bins + torch.randint(0, 2, (bins.numel(),), generator=gen)
    ids = _shuffled(rows.clamp(max=n_rows - 1), gen)

    counts = bc.bin_counts(ids, bits, n_rows)
    assert counts.numel() == MANY_BINS == 16422 and n_rows % 2 == 1
    assert torch.equal(counts, per_bin)
    assert -(-MANY_BINS // bc.SCAN_BLOCK) == 17
    assert counts[-1] == 1 and int(ids.max()) == n_rows - 1
    assert 0.05 < (counts == 0).float().mean() < 0.2
    for b in HEAVY_BLOCKS:
        assert b + 2 * stride < MANY_BINS
        assert 0 < counts[b] <= bc.hash_max_count(cap)
        assert counts[b + stride] > bc.hash_max_count(cap)
        assert 0 < counts[b + 2 * stride] <= bc.hash_max_count(cap)
        for r in (2 * b, 2 * b + 1):
            assert bc.home(r, cap) == bc.home(r + 4 * stride, cap)
    _case(kind, ids, n_rows, bits, gdtype, seed=8)


# ---- table boundaries ----------------------------------------------------------

@requires_gpu
@both_gdtypes
@pytest.mark.parametrize("bits", [7, 10])
@both_kinds
def test_boundary_rows(kind, bits, gdtype):
    """Five full bins and a last bin of one row; only row 0, the last row
    and the first and last row of every bin are updated.  Everything
    between, and the rows behind the table, stay as they were."""
    n_rows = 5 * 2 ** bits + 1
    n_bins = 6
    firsts = torch.arange(n_bins) << bits
    lasts = (firsts + 2 ** bits - 1).clamp(max=n_rows - 1)
    keys = torch.cat([torch.tensor([0, n_rows - 1]), firsts, lasts])
    gen = torch.Generator().manual_seed(bits)
    ids = _repeat_1_to_5(keys, gen)
    counts = bc.bin_counts(ids, bits, n_rows)
    assert counts.numel() == n_bins and (counts > 0).all()
    assert firsts[-1] == lasts[-1] == n_rows - 1  # the partial bin
    assert ids.unique().numel() == 2 * n_bins - 1
    _case(kind, ids, n_rows, bits, gdtype, seed=bits + 1)


# ---- which gradient an update reads --------------------------------------------

CODED_N = (1, 3, 67, 4099)


def _coded_check(kind, ids, n_rows, grad, per_update, gdtype):
    assert per_update.abs().max() <= exact_ints.BF16_INT_MAX
    assert ids.unique().numel() == ids.numel()
    want = torch.zeros(n_rows, per_update.shape[1])
    want[ids] = ALPHA * per_update.float()
    buf, view = _padded(torch.zeros_like(want))
    _launch(kind, view, ids.cuda(), grad.to(gdtype).cuda(), bits=7)
    got = buf.cpu()[:n_rows]
    bad = (got != want).any(dim=1).nonzero().reshape(-1)
    if bad.numel():
        update = {int(r): j for j, r in enumerate(ids.tolist())}
        r = int(bad[0])
        raise AssertionError(
            f"row {r} (update {update.get(r)}): got {got[r].tolist()}, "
            f"want {want[r].tolist()}; {bad.numel()} rows differ")
    _assert_table(buf, want, kind)


@requires_gpu
@both_gdtypes
@pytest.mark.parametrize("n", CODED_N)
def test_position_coded_deep(n, gdtype):
    """Distinct rows, zero table, ``grad[j, c] = (16 j + c) % 251 - 125``:
    every table entry names the update and column it must have come from,
    so a wrong ``j * DVEC + q`` or a quad taken from the neighbouring
    update shows, and the failure names the update."""
    n_rows = n + 904
    ids = torch.randperm(n_rows,
                         generator=torch.Generator().manual_seed(n))[:n]
    j = torch.arange(n).reshape(n, 1)
    c = torch.arange(DIM).reshape(1, DIM)
    grad = (16 * j + c) % 251 - 125
    _coded_check("deep", ids, n_rows, grad, grad, gdtype)


@requires_gpu
@both_gdtypes
@pytest.mark.parametrize("g_div", [1, 13, 26])
@pytest.mark.parametrize("n_out", CODED_N)
def test_position_coded_scalar(n_out, g_div, gdtype):
    """Update ``j`` of ``n_out * g_div`` reads ``gw[j // g_div]`` with
    ``gw[b] = b % 251 - 125``."""
    n = n_out * g_div
    n_rows = n + 904
    ids = torch.randperm(n_rows,
                         generator=torch.Generator().manual_seed(n))[:n]
    gw = torch.arange(n_out) % 251 - 125
    per_update = gw.repeat_interleave(g_div).reshape(n, 1)
    _coded_check("scalar", ids, n_rows, gw, per_update, gdtype)


# ---- one permutation for both tables -------------------------------------------

@requires_gpu
@both_gdtypes
def test_shared_permutation(gdtype):
    """The hand-over the module uses: one ``binned_permutation`` of the
    ``[B, F]`` ids serves the deep and the wide kernel as ``perm=``, and
    gives what ``perm=None`` gives.  A second launch on the updated
    tables with fresh gradients shows that nothing survives a launch."""
    B, F, n_rows, bits = 512, 13, 3000, 7
    n = B * F
    gen = torch.Generator().manual_seed(9)
    ids = torch.randint(0, n_rows, (B, F), generator=gen)
    _assert_exact(ids, launches=2)
    ids_gpu = ids.cuda()
    perm = ops.binned_permutation(ids_gpu, n_rows, bits)
    deep, g1, _ = _operands("deep", n, n_rows, seed=10)
    wide, gw1, gw1_per = _operands("scalar", n, n_rows, seed=11, g_div=F)
    _, g2, _ = _operands("deep", n, n_rows, seed=12)
    _, gw2, gw2_per = _operands("scalar", n, n_rows, seed=13, g_div=F)
    shared = (_padded(deep), _padded(wide))
    alone = (_padded(deep), _padded(wide))
    want_d, want_w = deep, wide
    for g, gw, gw_per in ((g1, gw1, gw1_per), (g2, gw2, gw2_per)):
        want_d = _ref(want_d, ids, g)
        want_w = _ref(want_w, ids, gw_per)
        g_gpu, gw_gpu = g.to(gdtype).cuda(), gw.to(gdtype).cuda()
        _launch("deep", shared[0][1], ids_gpu, g_gpu, perm=perm)
        _launch("scalar", shared[1][1], ids_gpu, gw_gpu, perm=perm)
        _launch("deep", alone[0][1], ids_gpu, g_gpu, bits=bits)
        _launch("scalar", alone[1][1], ids_gpu, gw_gpu, bits=bits)
        _assert_table(shared[0][0], want_d, "deep, shared perm")
        _assert_table(shared[1][0], want_w, "wide, shared perm")
        _assert_table(alone[0][0], want_d, "deep, own perm")
        _assert_table(alone[1][0], want_w, "wide, own perm")


@requires_gpu
@both_gdtypes
@pytest.mark.parametrize("bits", [7, None])
@both_kinds
def test_empty_update(kind, bits, gdtype):
    """No updates: the call returns and nothing is written."""
    n_rows = 300
    table, grad, _ = _operands(kind, 0, n_rows, seed=14)
    assert grad.numel() == 0
    buf, view = _padded(table)
    ids = torch.zeros(0, dtype=torch.int64)
    _launch(kind, view, ids.cuda(), grad.to(gdtype).cuda(), bits)
    _assert_table(buf, table.float(), kind)


# ---- pass A on its own -----------------------------------------------------------

# one trip of the count and slot kernels' grid-stride loops, plus three
ONE_TRIP = bc.PERM_GRID_MAX * bc.PERM_BLOCK


@requires_gpu
@pytest.mark.parametrize("n", [1, 255, 257, ONE_TRIP + 3])
@pytest.mark.parametrize("n_bins", [1, 2, 1023, 1024, 1025, 2049, 16422])
def test_permutation(n_bins, n):
    """``starts`` is the cumulative histogram (the scan at one bin, at
    one bin per thread, off by one either side, at 3 and at 17 bins per
    thread), ``order`` packs ``ids[j] << 31 | j`` for a permutation ``j``
    of the updates, and every slot of bin ``b`` holds a row of region
    ``b``.  The last bin has one row."""
    bits = 1
    n_rows = 2 * n_bins - 1
    gen = torch.Generator().manual_seed(n_bins + n)
    ids = torch.randint(0, n_rows, (n,), generator=gen)
    counts = bc.bin_counts(ids, bits, n_rows)
    assert counts.numel() == n_bins and ONE_TRIP == 2048 * 256
    order, starts = ops.binned_permutation(ids.cuda(), n_rows, bits)
    order, starts = order.cpu(), starts.cpu().long()
    want_starts = torch.cat([torch.zeros(1, dtype=torch.int64),
                             counts.cumsum(0)])
    assert torch.equal(starts, want_starts)
    assert order.shape == (n,)
    j = order & ((1 << bc.J_BITS) - 1)
    rows = order >> bc.J_BITS
    assert torch.equal(j.sort().values, torch.arange(n))
    assert torch.equal(rows, ids[j])
    bin_of_slot = torch.arange(n_bins).repeat_interleave(counts)
    assert torch.equal(rows >> bits, bin_of_slot)


# ---- the module's glue -------------------------------------------------------------

MOD_TABLES, MOD_B = [3000] * 4, 512


def _module_batch(law, gen):
    F = len(MOD_TABLES)
    if law == "uniform":
        ids = torch.randint(0, MOD_TABLES[0], (MOD_B, F), generator=gen)
    else:  # 64 rows per table: every row is hit about 8 times
        ids = torch.stack([
            torch.randperm(MOD_TABLES[f], generator=gen)[:64][
                torch.randint(0, 64, (MOD_B,), generator=gen)]
            for f in range(F)], dim=1)
        assert ids.unique().numel() <= 64 * F
    g_buf = exact_ints.ints((MOD_B, F * DIM), AMAX, gen)
    g_wide = exact_ints.ints((MOD_B,), AMAX, gen)
    return ids, g_buf, g_wide


class _ModuleRef:
    """float64 copies of both tables, updated as the module must."""

    def __init__(self, deep, wide):
        self.deep, self.wide = deep.double(), wide.double()
        self.offsets = torch.tensor(
            [sum(MOD_TABLES[:f]) for f in range(len(MOD_TABLES))])

    def forward(self, ids):
        flat = ids + self.offsets
        return (self.deep[flat].reshape(ids.shape[0], -1).float(),
                self.wide[flat].sum(dim=(1, 2)).float())

    def update(self, ids, g_buf, g_wide):
        flat = (ids + self.offsets).reshape(-1)
        F = ids.shape[1]
        self.deep.index_add_(0, flat, g_buf.double().reshape(-1, DIM),
                             alpha=ALPHA)
        self.wide.index_add_(
            0, flat, g_wide.double().repeat_interleave(F).reshape(-1, 1),
            alpha=ALPHA)


def _module_fwd_bwd(emb, ref, batch, perm_stream):
    """Forward (checked), backward with the batch's integer gradients;
    returns the address of the flat ids the sinks now hold."""
    ids, g_buf, g_wide = batch
    buf = torch.zeros(MOD_B, len(MOD_TABLES) * DIM, device="cuda")
    out, wide = emb(ids.cuda(), buf, 0)
    # the permutation was started in forward, on the side stream or inline
    key, _, event = emb._pending_perm
    assert (event is not None) == perm_stream
    want_out, want_wide = ref.forward(ids)
    assert torch.equal(out.detach().cpu(), want_out)
    assert torch.equal(wide.detach().cpu(), want_wide)
    n_sunk = len(emb._deep_sink)
    torch.autograd.backward([out, wide],
                            [g_buf.float().cuda(), g_wide.float().cuda()])
    assert len(emb._deep_sink) == len(emb._wide_sink) == n_sunk + 1
    assert emb._deep_sink[-1][0].data_ptr() == key
    return key


@requires_gpu
@pytest.mark.parametrize("steps", ["one", "two_steps",
                                   "two_forwards_one_apply"])
@pytest.mark.parametrize("law", ["uniform", "hot64"])
@pytest.mark.parametrize("perm_stream", [True, False],
                         ids=["side_stream", "inline"])
@pytest.mark.parametrize("apply_stream", [False, True],
                         ids=["apply_here", "apply_on_stream"])
def test_module_binned_path(monkeypatch, apply_stream, perm_stream, law,
                            steps):
    """``ShardedCriteoEmbeddings`` at world 1 with the binned scatter
    forced on: the permutation built during forward (side stream with its
    event, or inline) is handed to both kernels by the address of the ids,
    and the float64 ``index_add_`` of both tables comes back exactly.
    lr 0.5 at world 1 gives alpha = -0.5, and backward hands the integer
    gradients to the sinks unscaled, so nothing needs other values.
    apply_on_stream: ``apply_sparse_updates(lr, stream=S)`` runs both
    kernels on the caller's stream, a third stream for a permutation built
    on the side stream and a second for one built inline.
    two_steps: the second forward's ids may land on the freed address of
    the first's.  two_forwards_one_apply: only the second forward still
    has a pending permutation; the first's is built on demand."""
    from tf_yarn_amd.models.sharded_embedding import \
        ShardedCriteoEmbeddings
    monkeypatch.setenv("MIYARN_BINNED_SCATTER", "1")
    monkeypatch.setenv("MIYARN_PERM_STREAM", "1" if perm_stream else "0")
    gen = torch.Generator().manual_seed(15)
    rows = sum(MOD_TABLES)
    deep = exact_ints.ints((rows, DIM), AMAX, gen)
    wide = exact_ints.ints((rows, 1), AMAX, gen)
    emb = ShardedCriteoEmbeddings(MOD_TABLES, DIM).cuda()
    assert emb.world == 1
    with torch.no_grad():
        emb.weight.copy_(deep.float())
        emb.wide_weight.copy_(wide.float())
    ref = _ModuleRef(deep, wide)
    batches = [_module_batch(law, gen) for _ in range(2)]
    assert not torch.equal(batches[0][0], batches[1][0])
    # worst case: both batches hit one row MOD_B times each
    assert 2 * AMAX * MOD_B * abs(ALPHA) + AMAX < exact_ints.EXACT_LIMIT

    side = torch.cuda.Stream() if apply_stream else None

    def apply():
        emb.apply_sparse_updates(LR, stream=side)
        if side is not None:  # the caller's part of the hook's contract
            torch.cuda.current_stream().wait_stream(side)

    def check(what):
        torch.cuda.synchronize()
        assert emb._pending_perm is None
        assert not emb._deep_sink and not emb._wide_sink
        for got, want in ((emb.weight, ref.deep), (emb.wide_weight,
                                                   ref.wide)):
            got, want = got.detach().cpu(), want.float()
            bad = (got != want).any(dim=1).nonzero().reshape(-1)
            assert torch.equal(got, want), \
                f"{what}: rows {bad[:8].tolist()} of {tuple(got.shape)}"

    if steps == "two_forwards_one_apply":
        first = _module_fwd_bwd(emb, ref, batches[0], perm_stream)
        second = _module_fwd_bwd(emb, ref, batches[1], perm_stream)
        assert first != second and emb._pending_perm[0] == second
        apply()
        for batch in batches:
            ref.update(*batch)
        check("two forwards, one apply")
        return
    for step, batch in enumerate(batches[:1 if steps == "one" else 2]):
        _module_fwd_bwd(emb, ref, batch, perm_stream)
        apply()
        ref.update(*batch)
        check(f"step {step}")


@requires_gpu
def test_module_pending_permutation_lifetime(monkeypatch):
    """The pending permutation is matched to its ids by address, so it
    must not outlive them: a forward without grad starts none and drops an
    older one, and ``clear_pending`` drops it with the sinks."""
    from tf_yarn_amd.models.sharded_embedding import \
        ShardedCriteoEmbeddings
    monkeypatch.setenv("MIYARN_BINNED_SCATTER", "1")
    emb = ShardedCriteoEmbeddings(MOD_TABLES, DIM).cuda()
    ids = _module_batch("uniform", torch.Generator().manual_seed(16))[0]

    def forward():
        buf = torch.zeros(MOD_B, len(MOD_TABLES) * DIM, device="cuda")
        return emb(ids.cuda(), buf, 0)

    forward()
    assert emb._pending_perm is not None
    with torch.no_grad():
        forward()
    assert emb._pending_perm is None
    forward()
    assert emb._pending_perm is not None
    emb.clear_pending()
    assert emb._pending_perm is None
    torch.cuda.synchronize()
