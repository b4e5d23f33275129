"""Feature-sharded embeddings: exact parity with a single-process
replicated reference, over gloo world_size=2 (the all-to-all runs through
the gloo emulation; on GPU the same code takes RCCL all_to_all_single)."""

import pytest
import torch
import torch.multiprocessing as mp
from torch import nn

import exact_ints
from tf_yarn_amd.kv import KVClient, KVServer

F, D, ROWS, B, W = 4, 8, 50, 6, 2
TABLES = [ROWS] * F
LR = 0.25


def _global_tables(seed=123):
    g = torch.Generator().manual_seed(seed)
    deep = torch.randn(ROWS * F, D, generator=g)
    wide = torch.randn(ROWS * F, 1, generator=g) * 0.01
    return deep, wide


def _global_batch():
    g = torch.Generator().manual_seed(7)
    return torch.randint(0, ROWS, (W * B, F), generator=g)


def _reference():
    """Single-process full-table training step; returns (outputs
    [WB, F*D] in NATURAL feature order, wide [WB], updated tables)."""
    deep, wide = _global_tables()
    deep = deep.clone().requires_grad_(True)
    wide = wide.clone().requires_grad_(True)
    ids = _global_batch()
    offs = torch.arange(F) * ROWS
    flat = (ids + offs).reshape(-1)
    out = deep.index_select(0, flat).reshape(W * B, F * D)
    wide_out = wide.reshape(-1).index_select(0, flat).reshape(
        W * B, F).sum(dim=1)
    # global-mean loss over the whole (W*B) batch
    loss = out.float().pow(2).mean() + wide_out.float().pow(2).mean()
    loss.backward()
    new_deep = deep.detach() - LR * deep.grad
    new_wide = wide.detach() - LR * wide.grad
    return out.detach(), wide_out.detach(), new_deep, new_wide


def _shard_rows(table, rank):
    """Rows of the features rank owns (f % W == rank), feature-major."""
    parts = [table[f * ROWS:(f + 1) * ROWS] for f in range(F)
             if f % W == rank]
    return torch.cat(parts)


def _worker(rank, kv_addr, out_q):
    from tf_yarn_amd.models.sharded_embedding import \
        ShardedCriteoEmbeddings
    from tf_yarn_amd.parallel import comm
    client = KVClient(kv_addr)
    comm.init_process_group(rank=rank, world_size=W, backend="gloo",
                            kv_client=client)
    try:
        emb = ShardedCriteoEmbeddings(TABLES, D)
        deep, wide = _global_tables()
        emb.weight.data.copy_(_shard_rows(deep, rank))
        emb.wide_weight.data.copy_(_shard_rows(wide, rank))
        ids = _global_batch()[rank * B:(rank + 1) * B]
        buf = torch.zeros(B, F * D)
        out_buf, wide_out = emb(ids, buf, 0)
        # local-mean loss; global equivalence needs the 1/W apply scale
        loss = out_buf.float().pow(2).mean() \
            + wide_out.float().pow(2).mean()
        loss.backward()
        emb.apply_sparse_updates(LR)
        out_q.put((rank,
                   out_buf.detach().numpy().copy(),
                   wide_out.detach().numpy().copy(),
                   emb.weight.detach().numpy().copy(),
                   emb.wide_weight.detach().numpy().copy()))
    finally:
        comm.destroy_process_group()


@pytest.mark.timeout(180)
def test_sharded_matches_replicated_reference():
    server = KVServer()
    ctx = mp.get_context("spawn")
    out_q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, server.address, out_q))
             for r in range(W)]
    for p in procs:
        p.start()
    try:
        results = {}
        for _ in range(W):
            r, out, wide, dw, ww = out_q.get(timeout=150)
            results[r] = (torch.from_numpy(out), torch.from_numpy(wide),
                          torch.from_numpy(dw), torch.from_numpy(ww))
    finally:
        for p in procs:
            p.join(timeout=30)
            if p.is_alive():
                p.terminate()
        server.stop()

    ref_out, ref_wide, ref_deep, ref_wide_t = _reference()
    # owner-permuted feature order: [f for s in range(W) for f owned by s]
    perm = [f for s in range(W) for f in range(F) if f % W == s]
    for r in range(W):
        out, wide, dw, ww = results[r]
        ref_r = ref_out[r * B:(r + 1) * B].reshape(B, F, D)
        expect = ref_r[:, perm, :].reshape(B, F * D)
        assert torch.allclose(out, expect, atol=1e-5), \
            f"rank {r} forward mismatch"
        assert torch.allclose(wide, ref_wide[r * B:(r + 1) * B],
                              atol=1e-5), f"rank {r} wide mismatch"
        assert torch.allclose(dw, _shard_rows(ref_deep, r), atol=1e-5), \
            f"rank {r} deep update mismatch"
        assert torch.allclose(ww, _shard_rows(ref_wide_t, r),
                              atol=1e-5), f"rank {r} wide update mismatch"


def test_sharded_local_world1_matches_replicated():
    """W == 1 path equals the plain local computation."""
    from tf_yarn_amd.models.sharded_embedding import \
        ShardedCriteoEmbeddings
    emb = ShardedCriteoEmbeddings(TABLES, D)
    deep, wide = _global_tables()
    emb.weight.data.copy_(deep)
    emb.wide_weight.data.copy_(wide)
    ids = _global_batch()[:B]
    buf = torch.zeros(B, F * D)
    out_buf, wide_out = emb(ids, buf, 0)
    offs = torch.arange(F) * ROWS
    flat = (ids + offs).reshape(-1)
    ref = deep.index_select(0, flat).reshape(B, F * D)
    ref_wide = wide.reshape(-1).index_select(0, flat).reshape(
        B, F).sum(dim=1)
    assert torch.allclose(out_buf, ref, atol=1e-5)
    assert torch.allclose(wide_out, ref_wide, atol=1e-5)
    # backward + apply runs
    (out_buf.pow(2).mean() + wide_out.pow(2).mean()).backward()
    emb.apply_sparse_updates(0.1)


def _worker4(rank, kv_addr, out_q):
    from tf_yarn_amd.models.sharded_embedding import \
        ShardedCriteoEmbeddings
    from tf_yarn_amd.parallel import comm
    client = KVClient(kv_addr)
    comm.init_process_group(rank=rank, world_size=4, backend="gloo",
                            kv_client=client)
    try:
        import torch as t
        emb = ShardedCriteoEmbeddings([20] * 6, 4)  # 6 feats / 4 ranks
        g = t.Generator().manual_seed(11)
        full = t.randn(120, 4, generator=g)
        own = t.cat([full[f * 20:(f + 1) * 20]
                     for f in range(6) if f % 4 == rank])
        emb.weight.data.copy_(own)
        ids = t.randint(0, 20, (3, 6),
                        generator=t.Generator().manual_seed(rank))
        buf = t.zeros(3, 24)
        out_buf, wide = emb(ids, buf, 0)
        # reference: local gather on the full table (perm feature order)
        offs = t.arange(6) * 20
        perm = [f for s in range(4) for f in range(6) if f % 4 == s]
        flat = (ids + offs)[:, perm].reshape(-1)
        ref = full.index_select(0, flat).reshape(3, 24)
        out_q.put((rank, bool(t.allclose(out_buf, ref, atol=1e-5))))
    finally:
        comm.destroy_process_group()


@pytest.mark.timeout(180)
def test_sharded_forward_world4_uneven_features():
    """6 features over 4 ranks (2,2,1,1): uneven alltoall splits."""
    server = KVServer()
    ctx = mp.get_context("spawn")
    out_q = ctx.Queue()
    procs = [ctx.Process(target=_worker4, args=(r, server.address, out_q))
             for r in range(4)]
    for p in procs:
        p.start()
    try:
        results = dict(out_q.get(timeout=150) for _ in range(4))
    finally:
        for p in procs:
            p.join(timeout=30)
            if p.is_alive():
                p.terminate()
        server.stop()
    assert all(results.values()), results


# ---- one record per backward (world 1) -------------------------------------

def _int_tables(emb, gen):
    """Integer-valued tables in ``emb``; their float64 copies."""
    deep = exact_ints.ints((ROWS * F, D), 4, gen)
    wide = exact_ints.ints((ROWS * F, 1), 4, gen)
    emb.weight.data.copy_(deep.float())
    emb.wide_weight.data.copy_(wide.float())
    return deep.double(), wide.double()


@pytest.mark.parametrize("order", ["a_then_b", "b_then_a"])
def test_two_forwards_at_different_col_offsets(order):
    """Forward A fills a buffer from column 0, forward B one from column 16
    behind the dense columns; each backward must slice ITS buffer's
    gradient at its own forward's ``col_offset``, whichever runs first.
    Integer operands and lr 0.5: the float64 ``index_add_`` of both tables
    comes back exactly."""
    from tf_yarn_amd.models.sharded_embedding import \
        ShardedCriteoEmbeddings
    b, lr, pad = 32, 0.5, 16
    gen = torch.Generator().manual_seed(31)
    emb = ShardedCriteoEmbeddings(TABLES, D)
    assert emb.world == 1
    want_deep, want_wide = _int_tables(emb, gen)
    assert 2 * 4 * b * lr + 4 < exact_ints.EXACT_LIMIT
    offs = torch.arange(F) * ROWS
    runs = {}
    for name, col in (("a", 0), ("b", pad)):
        ids = torch.randint(0, ROWS, (b, F), generator=gen)
        buf = torch.zeros(b, col + F * D)
        dense = torch.randn(b, 13, generator=gen) if col else None
        out, wide_out = emb(ids, buf, col, dense=dense)
        g_buf = exact_ints.ints((b, col + F * D), 4, gen)
        g_wide = exact_ints.ints((b,), 4, gen)
        runs[name] = (out, wide_out, g_buf.float(), g_wide.float())
        flat = (ids + offs).reshape(-1)
        want_deep.index_add_(0, flat,
                             g_buf[:, col:].double().reshape(-1, D),
                             alpha=-lr)
        want_wide.index_add_(
            0, flat, g_wide.double().repeat_interleave(F).reshape(-1, 1),
            alpha=-lr)
    for name in (("a", "b") if order == "a_then_b" else ("b", "a")):
        out, wide_out, g_buf, g_wide = runs[name]
        torch.autograd.backward([out, wide_out], [g_buf, g_wide])
    assert len(emb.pending_grads()) == 2
    emb.apply_sparse_updates(lr)
    assert not emb.pending_grads()
    assert torch.equal(emb.weight.detach(), want_deep.float())
    assert torch.equal(emb.wide_weight.detach(), want_wide.float())


@pytest.mark.parametrize("deep_rule,wide_rule",
                         [("adagrad", "adagrad"), ("adagrad", "ftrl"),
                          ("lazy_adam", "lazy_adam")])
def test_each_record_applies_its_own_pair(deep_rule, wide_rule, monkeypatch):
    """Two forwards and backwards, one apply, two stateful tables: every
    record goes to ``ops.emb_bwd_sparse`` once, as a pair whose two sides
    carry the gradients of that record, in the records' order."""
    from tf_yarn_amd import ops
    from tf_yarn_amd.models.sharded_embedding import \
        ShardedCriteoEmbeddings
    b = 32
    gen = torch.Generator().manual_seed(32)
    torch.manual_seed(33)
    emb = ShardedCriteoEmbeddings(TABLES, D, sparse_optimizer=deep_rule,
                                  wide_sparse_optimizer=wide_rule)
    for _ in range(2):
        ids = torch.randint(0, ROWS, (b, F), generator=gen)
        out, wide_out = emb(ids, torch.zeros(b, F * D), 0)
        torch.autograd.backward(
            [out, wide_out], [torch.randn(b, F * D, generator=gen),
                              torch.randn(b, generator=gen)])
    want = [(r.ids, r.deep_grad.clone(), r.wide_grad.clone())
            for r in emb.pending_grads()]
    assert len(want) == 2
    assert not torch.equal(want[0][1], want[1][1])
    assert not torch.equal(want[0][2], want[1][2])
    calls = []
    real = ops.emb_bwd_sparse

    def recorder(ids, *, deep=None, wide=None, **kw):
        calls.append((ids, deep, wide))
        return real(ids, deep=deep, wide=wide, **kw)

    monkeypatch.setattr(ops, "emb_bwd_sparse", recorder)
    emb.apply_sparse_updates(LR)
    assert len(calls) == 2
    for (ids, deep, wide), (w_ids, w_deep, w_wide) in zip(calls, want):
        assert ids is w_ids
        assert (deep.rule, wide.rule) == (deep_rule, wide_rule)
        assert torch.equal(deep.grad.reshape(b, F * D), w_deep)
        assert torch.equal(wide.grad, w_wide)
    if deep_rule == "lazy_adam":
        assert emb.adam_step_count("") == 2
        assert emb.adam_step_count("wide_") == 2
