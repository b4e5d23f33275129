"""Bit-exact tests of the single-GPU sparse path from RAW ids.

``emb_lookup_fused`` (offset add + deep gather into the MLP-input slice +
wide gather-sum + dense / pad columns, one kernel) must reproduce the
separate ops it replaces to the bit, the wide sum included: it adds the
same fp32 scalars in the same order.  ``emb_bwd_sgd_fused_wide`` with
``offsets`` must leave the tables it leaves from pre-added ids.  At model
level, two training steps with MIYARN_FUSED_LOOKUP / MIYARN_FUSED_HEAD_BWD
on and off must give the same loss and parameters.

Every comparison is ``torch.equal``.  Where atomics could reorder float
sums (duplicate ids in a scatter) the operands are the small integers of
exact_ints.py, for which every order gives the same sum.
"""

import pytest
import torch

import exact_ints
from tf_yarn_amd import ops

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")

F32, BF16 = torch.float32, torch.bfloat16
# launch arithmetic of emb_lookup_fused (embedding.hip): a block owns
# chunks of min(32, 2048 // F) batch rows, at most 2048 blocks
CHUNK_ROWS, MAX_BLOCKS = 32, 2048


def _offsets(f, rows_per_feature, shared):
    """Per-feature row offsets; ``shared``: all features use ONE table, so
    a batch row can name the same table row more than once."""
    if shared:
        return torch.zeros(f, dtype=torch.int64)
    return torch.arange(f, dtype=torch.int64) * rows_per_feature


def _lookup_operands(b, f, dim, n_dense, rows_per_feature, shared, seed):
    gen = torch.Generator().manual_seed(seed)
    n_rows = rows_per_feature * (1 if shared else f)
    table = torch.randn(n_rows, dim, generator=gen)
    wide = torch.randn(n_rows, 1, generator=gen)
    ids = torch.randint(0, rows_per_feature, (b, f), generator=gen)
    dense = torch.randn(b, n_dense, generator=gen)
    return (table.cuda(), wide.cuda(), ids.cuda(),
            _offsets(f, rows_per_feature, shared).cuda(), dense.cuda())


def _separate_ops(table, wide, ids, offsets, dense, out, col_offset):
    """What the model ran before the fused kernel: ``ids + offsets``,
    ``emb_fwd_into`` (``emb_fwd`` + a copy where that op does not take
    the shape), ``emb_gather_sum``, the two fills."""
    b, f = ids.shape
    dim = table.shape[1]
    bf16 = out.dtype == BF16
    flat = (ids + offsets.unsqueeze(0)).reshape(-1)
    if dim % 4 == 0 and col_offset % 4 == 0 and out.shape[1] % 4 == 0:
        ops.emb_fwd_into(table, flat, out, col_offset)
    else:
        out[:, col_offset:col_offset + f * dim] = \
            ops.emb_fwd(table, flat, bf16).reshape(b, f * dim)
    wide_sum = ops.emb_gather_sum(wide, flat.reshape(b, f), bf16)
    n_dense = dense.shape[1]
    out[:, :n_dense] = dense
    out[:, n_dense:col_offset] = 0
    return wide_sum


# (b, f, dim, n_dense, col_offset, extra out cols, rows/feature, shared)
LOOKUP_CASES = {
    "b1_f1": (1, 1, 16, 0, 0, 0, 7, False),
    "model_layout": (5, 26, 16, 13, 16, 0, 300, False),
    "dim4_ragged_chunk": (37, 3, 4, 3, 4, 0, 50, False),
    "dim64": (33, 2, 64, 5, 8, 0, 20, False),
    "no_dense_no_offset": (64, 4, 8, 0, 0, 0, 11, False),
    "untouched_tail_cols": (9, 2, 8, 2, 4, 8, 11, False),
    # 2048 // 100 = 20 rows per chunk instead of 32; 3 chunks, last ragged
    "many_features": (45, 100, 4, 0, 0, 0, 6, False),
    # same table row within a batch row and across batch rows
    "repeated_ids": (40, 6, 16, 13, 16, 0, 3, True),
    # more chunks than blocks: the first 2 blocks take a second chunk, the
    # last of them ragged
    "grid_wrap": (CHUNK_ROWS * MAX_BLOCKS + 37, 2, 4, 1, 4, 0, 5, False),
}


@requires_gpu
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", sorted(LOOKUP_CASES))
def test_lookup_fused_matches_separate_ops(case, dtype):
    b, f, dim, n_dense, col_offset, extra, rpf, shared = LOOKUP_CASES[case]
    table, wide, ids, offsets, dense = _lookup_operands(
        b, f, dim, n_dense, rpf, shared, seed=len(case))
    dense = dense.to(dtype)
    cols = col_offset + f * dim + extra
    want = torch.full((b, cols), 3.0, dtype=dtype, device="cuda")
    got = want.clone()
    assert ops.emb_lookup_fused_covers(table, ids, dense, got, col_offset)
    want_wide = _separate_ops(table, wide, ids, offsets, dense, want,
                              col_offset)
    got_wide = ops.emb_lookup_fused(table, wide, ids, offsets, dense, got,
                                    col_offset)
    assert got_wide.dtype == want_wide.dtype == dtype
    assert torch.equal(got, want)
    assert torch.equal(got_wide, want_wide)


@requires_gpu
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("dim,col_offset", [(7, 4), (16, 2)],
                         ids=["dim7", "col_offset2"])
def test_lookup_fused_fallback_shapes(dim, col_offset, dtype):
    """Shapes the kernel does not take go through the separate ops."""
    b, f, n_dense = 21, 5, 1
    table, wide, ids, offsets, dense = _lookup_operands(
        b, f, dim, n_dense, 30, False, seed=dim)
    dense = dense.to(dtype)
    want = torch.full((b, col_offset + f * dim), 3.0, dtype=dtype,
                      device="cuda")
    got = want.clone()
    assert not ops.emb_lookup_fused_covers(table, ids, dense, got,
                                           col_offset)
    want_wide = _separate_ops(table, wide, ids, offsets, dense, want,
                              col_offset)
    got_wide = ops.emb_lookup_fused(table, wide, ids, offsets, dense, got,
                                    col_offset)
    assert torch.equal(got, want)
    assert torch.equal(got_wide, want_wide)


# ---- scatter with in-kernel offsets ----------------------------------------

LR, SCALE = 0.5, 1.0  # alpha = -0.5: a power of two
AMAX = 4


def _grad_views(grad2d, b, f, dim, strided):
    """The [b*f, dim] gradient as the op takes it: dense, or the column
    slice ``[:, 16:]`` of a ``[b, 16 + f*dim]`` buffer."""
    if not strided:
        return grad2d.clone()
    buf = torch.zeros(b, 16 + f * dim, dtype=grad2d.dtype,
                      device=grad2d.device)
    buf[:, 16:] = grad2d.reshape(b, f * dim)
    return buf[:, 16:]


def _scatter_both(table, wide, ids, offsets, grad2d, gw, strided):
    """(deep, wide) after the update from raw ids + offsets, and after the
    update from pre-added ids."""
    b, f = ids.shape
    dim = table.shape[1]
    out = []
    for raw in (True, False):
        t, w = table.clone(), wide.clone()
        g = _grad_views(grad2d, b, f, dim, strided)
        if raw:
            ops.emb_bwd_sgd_fused_wide(t, w, ids, g, gw, lr=LR, scale=SCALE,
                                       offsets=offsets)
        else:
            flat = (ids + offsets.unsqueeze(0)).reshape(-1)
            ops.emb_bwd_sgd_fused_wide(t, w, flat, g, gw, lr=LR,
                                       scale=SCALE)
        out.append((t, w))
    return out


@requires_gpu
@pytest.mark.parametrize("strided", [False, True], ids=["dense", "slice"])
@pytest.mark.parametrize("gdtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("dim", [16, 8])  # the dim-16 and runtime-dim kernels
def test_scatter_offsets_distinct_ids(dim, gdtype, strided):
    """No table row named twice: one add per entry, so random floats
    compare exactly."""
    b, f, rpf = 64, 5, 64
    gen = torch.Generator().manual_seed(dim)
    ids = torch.stack([torch.randperm(rpf, generator=gen)[:b]
                       for _ in range(f)], dim=1).cuda()
    offsets = _offsets(f, rpf, False).cuda()
    table = torch.randn(f * rpf, dim, generator=gen).cuda()
    wide = torch.randn(f * rpf, 1, generator=gen).cuda()
    grad = torch.randn(b * f, dim, generator=gen).to(gdtype).cuda()
    gw = torch.randn(b, generator=gen).to(gdtype).cuda()
    (t_raw, w_raw), (t_flat, w_flat) = _scatter_both(
        table, wide, ids, offsets, grad, gw, strided)
    assert not torch.equal(t_raw, table)  # something was written
    assert torch.equal(t_raw, t_flat)
    assert torch.equal(w_raw, w_flat)


@requires_gpu
@pytest.mark.parametrize("strided", [False, True], ids=["dense", "slice"])
@pytest.mark.parametrize("gdtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("dim", [16, 8])
def test_scatter_offsets_heavy_duplicates_exact(dim, gdtype, strided):
    """3 rows per feature, 3001 examples: ~1000 adds per table row.
    Integer operands and alpha = -0.5 keep every sum exact in any order,
    so both calls must hit the float64 reference bit for bit."""
    b, f, rpf = 3001, 26, 3
    assert AMAX * b * f * LR * SCALE + AMAX < exact_ints.EXACT_LIMIT
    gen = torch.Generator().manual_seed(dim + 1)
    ids = torch.randint(0, rpf, (b, f), generator=gen)
    offsets = _offsets(f, rpf, False)
    table = exact_ints.ints((f * rpf, dim), AMAX, gen)
    wide = exact_ints.ints((f * rpf, 1), AMAX, gen)
    grad = exact_ints.ints((b * f, dim), AMAX, gen)
    gw = exact_ints.ints((b,), AMAX, gen)
    flat = (ids + offsets.unsqueeze(0)).reshape(-1)
    want_t = table.double().index_add_(0, flat, grad.double(),
                                       alpha=-LR * SCALE).float()
    want_w = wide.double().index_add_(
        0, flat, gw.double().repeat_interleave(f).reshape(-1, 1),
        alpha=-LR * SCALE).float()
    (t_raw, w_raw), (t_flat, w_flat) = _scatter_both(
        table.to(F32).cuda(), wide.to(F32).cuda(), ids.cuda(),
        offsets.cuda(), grad.to(gdtype).cuda(), gw.to(gdtype).cuda(),
        strided)
    assert torch.equal(t_raw.cpu(), want_t)
    assert torch.equal(w_raw.cpu(), want_w)
    assert torch.equal(t_flat.cpu(), want_t)
    assert torch.equal(w_flat.cpu(), want_w)


# ---- model level -----------------------------------------------------------

def _train_two_steps(monkeypatch, switch):
    from tf_yarn_amd.models.wide_deep import WideAndDeep
    from tf_yarn_amd.ops.optim import FusedSGD
    monkeypatch.setenv("MIYARN_FUSED_LOOKUP", switch)
    monkeypatch.setenv("MIYARN_FUSED_HEAD_BWD", switch)
    monkeypatch.setenv("MIYARN_BINNED_SCATTER", "0")
    f, rpf, b = 26, 80, 64
    torch.manual_seed(3)
    model = WideAndDeep(table_sizes=[rpf] * f, embedding_dim=16,
                        hidden=(64, 32), compute_dtype=BF16,
                        sharded=True).cuda()
    opt = FusedSGD([p for p in model.parameters()
                    if not getattr(p, "_miyarn_sparse", False)], lr=0.05)
    gen = torch.Generator().manual_seed(4)
    losses, raw_entries, head_calls = [], [], []
    real_head = ops.linear_bias_relu_head
    monkeypatch.setattr(ops, "linear_bias_relu_head",
                        lambda *a: head_calls.append(1) or real_head(*a))
    for _ in range(2):
        # no table row named twice in a batch: scatter order cannot matter
        ids = torch.stack([torch.randperm(rpf, generator=gen)[:b]
                           for _ in range(f)], dim=1).cuda()
        dense = torch.randn(b, 13, generator=gen).cuda()
        labels = torch.randint(0, 2, (b,), generator=gen).float().cuda()
        opt.zero_grad(set_to_none=True)
        loss = model(dense, ids, labels=labels)
        loss.backward()
        raw_entries.append(len(model.embeddings._raw_ids_keys))
        opt.step()
        model.apply_sparse_updates(lr=0.05)
        losses.append(loss.detach().clone())
    torch.cuda.synchronize()
    return model, losses, raw_entries, len(head_calls)


@requires_gpu
def test_model_two_steps_switches_on_equal_off(monkeypatch):
    on, on_losses, on_raw, on_head = _train_two_steps(monkeypatch, "1")
    off, off_losses, off_raw, off_head = _train_two_steps(monkeypatch, "0")
    # the switches select the paths they name
    assert on_raw == [1, 1] and on_head == 2
    assert off_raw == [0, 0] and off_head == 0
    for a, c in zip(on_losses, off_losses):
        assert torch.equal(a, c)
    assert list(on.state_dict()) == list(off.state_dict())
    for (name, p), (_, q) in zip(on.named_parameters(),
                                 off.named_parameters()):
        assert torch.equal(p, q), name
