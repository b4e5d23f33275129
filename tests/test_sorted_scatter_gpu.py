"""Exact tests of the sorted segmented scatter (``_C.emb_bwd_sgd_sorted``,
embedding.hip).

The ids arrive sorted; the thread that holds the first update of a run
(and one quad of the row) adds the whole run with a plain read-modify-
write, every other thread of the run adds nothing, and there are no
atomics.  Tables and gradients are small integers and ``alpha = -0.5``, so
the float64 ``index_add_`` reference must come back bit for bit (see
exact_ints.py): a run cut short at a block or grid-trip edge, a second
add by a non-head thread or a quad from the neighbouring update moves an
integer sum and fails ``torch.equal``.  The whole table is compared.
"""

import pytest
import torch

import exact_ints

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")

F32, BF16 = torch.float32, torch.bfloat16
both_gdtypes = pytest.mark.parametrize("gdtype", [F32, BF16],
                                       ids=["f32", "bf16"])
AMAX = 4
LR, SCALE = 0.5, 1.0
ALPHA = -LR * SCALE

# launch arithmetic of emb_bwd_sgd_sorted (embedding.hip): one quad of one
# update per thread per trip, MIYARN_BLOCK = 256 threads, at most 8192
# blocks (``miyarn_grid_cap(n * (dim / 4), 8192)``).  The extension does
# not report these, so this copy is kept in step BY HAND: if the block
# size or the cap changes there, change it here, or the two edge cases
# below stop sitting on their edges while still passing.
BLOCK, GRID_MAX = 256, 8192

DIMS = (4, 16, 64, 128)
# off the wave (1, 3), off the block (67), many blocks with a ragged last
# one (70001; at dim 128 more than one grid trip)
TAILS = (1, 3, 67, 70001)


def _sorted_ids(law, n, gen):
    if law == "distinct":  # every thread is a head
        ids = torch.randperm(n + 50, generator=gen)[:n].sort().values
        assert ids.unique().numel() == n
    elif law == "one_run":  # one head per quad adds all n updates
        ids = torch.full((n,), 7)
    elif law == "random_runs":  # run lengths around 5, some rows skipped
        ids = torch.randint(0, max(1, n // 5), (n,),
                            generator=gen).sort().values
        assert n < 10 or ids.unique().numel() < n
    else:  # "pairs": runs of 2 (a last run of 1 at odd n), with gaps
        ids = 3 * (torch.arange(n) // 2)
        assert n < 2 or torch.bincount(ids).max() == 2
    assert torch.equal(ids, ids.sort().values)
    return ids


def _check(ids, dim, gdtype, seed):
    import tf_yarn_amd.ops._C as C
    n = ids.numel()
    rows = int(ids.max()) + 3
    # worst case: every update lands on one entry; the run is summed
    # before it is scaled
    assert AMAX * n < exact_ints.EXACT_LIMIT
    assert AMAX * n * abs(ALPHA) + AMAX < exact_ints.EXACT_LIMIT
    gen = torch.Generator().manual_seed(seed)
    table = exact_ints.ints((rows, dim), AMAX, gen)
    grad = exact_ints.ints((n, dim), AMAX, gen)
    want = table.double()
    want.index_add_(0, ids, grad.double(), alpha=ALPHA)
    want = want.float()
    t = table.float().cuda()
    C.emb_bwd_sgd_sorted(t, ids.cuda(), grad.to(gdtype).cuda(), LR, SCALE)
    got = t.cpu()
    bad = (got != want).any(dim=1).nonzero().reshape(-1)
    assert torch.equal(got, want), (
        f"{bad.numel()} rows differ, first {bad[:8].tolist()} "
        f"(updates {(ids == bad[0]).nonzero().reshape(-1)[:4].tolist()})")


@requires_gpu
@both_gdtypes
@pytest.mark.parametrize("law", ["distinct", "one_run", "random_runs",
                                 "pairs"])
@pytest.mark.parametrize("n", TAILS)
@pytest.mark.parametrize("dim", DIMS)
def test_run_laws(dim, n, law, gdtype):
    """1 to 32 quads per update, sizes off the wave and off the block, and
    every mix of head and non-head threads: all heads, one head per quad
    with a run of n behind it, random runs, and head / non-head
    alternating."""
    gen = torch.Generator().manual_seed(dim + n)
    _check(_sorted_ids(law, n, gen), dim, gdtype, seed=dim * 3 + n)


@requires_gpu
@both_gdtypes
def test_run_crosses_block_edge(gdtype):
    """dim 16 is 4 quads per update, 64 updates per block: the run over
    updates 63 and 64 starts in the last threads of block 0 and goes on in
    block 1, whose first threads must add nothing."""
    dim, n = 16, 131
    per_block = BLOCK // (dim // 4)
    assert per_block == 64
    ids = 2 * torch.arange(n)
    ids[64] = ids[63]
    assert 63 // per_block == 0 and 64 // per_block == 1
    assert torch.bincount(ids).max() == 2
    _check(ids, dim, gdtype, seed=1)


@requires_gpu
@both_gdtypes
def test_run_straddles_grid_trip(gdtype):
    """dim 128 is 32 quads per update, so one trip of the capped grid
    covers 65536 updates: the run over updates 65534 to 65537 starts at
    the end of the first trip and its other half belongs to threads of
    the second trip, which must add nothing."""
    dim, n = 128, 65536 + 5
    per_trip = GRID_MAX * BLOCK // (dim // 4)
    assert per_trip == 65536 and per_trip < n
    ids = torch.arange(n)
    ids[65534:65538] = ids[65534]
    assert (ids == ids[65534]).nonzero().reshape(-1).tolist() == \
        [65534, 65535, 65536, 65537]
    assert torch.equal(ids, ids.sort().values)
    _check(ids, dim, gdtype, seed=2)
