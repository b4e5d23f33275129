"""Sparse Adagrad for the embedding tables: the reference op against
torch.optim.Adagrad, duplicate coalescing, untouched rows, and the model
wiring (replicated, sharded, checkpoints, 2-rank gloo)."""

import copy

import pytest
import torch
import torch.multiprocessing as mp
from torch import nn

from tf_yarn_amd import ops
from tf_yarn_amd.kv import KVClient, KVServer
from tf_yarn_amd.models.wide_deep import (FlatInputWideAndDeep,
                                          SparseEmbedding, WideAndDeep,
                                          WideScalarEmbedding)

LR = 0.05


@pytest.mark.parametrize("dim", [16, 1])
def test_reference_matches_torch_adagrad(dim):
    torch.manual_seed(0)
    emb = nn.Embedding(300, dim, sparse=True)
    opt = torch.optim.Adagrad(emb.parameters(), lr=LR)
    table = emb.weight.detach().clone()
    state = torch.zeros_like(table)
    for step in range(3):
        ids = torch.randint(0, 40, (64,))  # heavy overlap within + across
        grad_out = torch.randn(64, dim)
        opt.zero_grad()
        emb(ids).backward(grad_out)
        opt.step()
        ops.emb_bwd_adagrad(table, state, ids, grad_out, lr=LR)
        assert torch.allclose(table, emb.weight.detach(), atol=1e-6), step
    assert torch.allclose(state, opt.state[emb.weight]["sum"], atol=1e-6)


def test_wide_companion_matches_torch_adagrad():
    torch.manual_seed(1)
    f = 4
    emb = nn.Embedding(300, 1, sparse=True)
    opt = torch.optim.Adagrad(emb.parameters(), lr=LR)
    table = emb.weight.detach().clone()
    state = torch.zeros_like(table)
    for _ in range(3):
        ids = torch.randint(0, 40, (16, f))
        gw = torch.randn(16)
        opt.zero_grad()
        emb(ids).sum(dim=(1, 2)).backward(gw)
        opt.step()
        ops.emb_bwd_adagrad_wide(table, state, ids, gw, lr=LR)
        assert torch.allclose(table, emb.weight.detach(), atol=1e-6)


def test_duplicates_are_coalesced_before_the_state_update():
    torch.manual_seed(2)
    dim, eps, scale = 4, 1e-10, 0.5
    table = torch.randn(10, dim)
    state = torch.full((10, dim), 0.25)
    rows = torch.tensor([2, 5, 7])
    ids = rows[torch.arange(512) % 3]
    grad = torch.randint(-32, 33, (512, dim)).float() / 8
    expect_t, expect_s = table.clone(), state.clone()
    for k, r in enumerate(rows.tolist()):
        g = scale * grad[k::3].sum(dim=0)
        expect_s[r] += g * g
        expect_t[r] -= LR * g / (expect_s[r].sqrt() + eps)
    ops.emb_bwd_adagrad(table, state, ids, grad, lr=LR, eps=eps,
                        scale=scale)
    assert torch.allclose(table, expect_t, atol=1e-6)
    assert torch.allclose(state, expect_s, atol=1e-6)


def test_untouched_rows_are_bit_identical():
    torch.manual_seed(3)
    table = torch.randn(100, 16)
    state = torch.rand(100, 16)
    t0, s0 = table.clone(), state.clone()
    ids = torch.randint(0, 50, (200,)) * 2  # even rows only
    ops.emb_bwd_adagrad(table, state, ids, torch.randn(200, 16), lr=LR)
    odd = torch.arange(1, 100, 2)
    assert torch.equal(table[odd], t0[odd])
    assert torch.equal(state[odd], s0[odd])
    touched = torch.unique(ids)
    assert not torch.equal(table[touched], t0[touched])


def test_fused_wide_equals_the_two_single_table_ops():
    torch.manual_seed(4)
    n, f, dim = 96, 4, 16
    ids = torch.randint(0, 30, (n,))
    grad, gw = torch.randn(n, dim), torch.randn(n // f)
    t1, s1 = torch.randn(60, dim), torch.zeros(60, dim)
    w1, ws1 = torch.randn(60, 1), torch.zeros(60, 1)
    t2, s2, w2, ws2 = t1.clone(), s1.clone(), w1.clone(), ws1.clone()
    ops.emb_bwd_adagrad_fused_wide(t1, s1, w1, ws1, ids, grad, gw, lr=LR)
    ops.emb_bwd_adagrad(t2, s2, ids, grad, lr=LR)
    ops.emb_bwd_adagrad_wide(w2, ws2, ids, gw, lr=LR)
    assert torch.equal(t1, t2) and torch.equal(s1, s2)
    assert torch.equal(w1, w2) and torch.equal(ws1, ws2)


# ---- model wiring ----------------------------------------------------------

TABLES = [50] * 4


def _model(**kw):
    return WideAndDeep(table_sizes=TABLES, embedding_dim=4, hidden=(8,),
                       sparse_optimizer="adagrad", **kw)


def _batch(seed, b=32):
    g = torch.Generator().manual_seed(seed)
    dense = torch.randn(b, 13, generator=g)
    ids = torch.randint(0, 12, (b, len(TABLES)), generator=g)
    labels = torch.rand(b, generator=g).round()
    return dense, ids, labels


def _tables(model):
    if model.sharded:
        e = model.embeddings
        return e.weight, e.state_sum, e.wide_weight, e.wide_state_sum
    d, w = model.deep_embedding, model.wide_embedding
    return d.weight, d.state_sum, w.weight, w.state_sum


def _sinks(model):
    if model.sharded:
        return model.embeddings._deep_sink, model.embeddings._wide_sink
    return (model.deep_embedding.pending_grads(),
            model.wide_embedding.pending_grads())


def _step_and_check(model, seed):
    """backward, read the sinks, apply through the model and through the
    reference op on copies; both must agree."""
    dense, ids, labels = _batch(seed)
    model(dense, ids, labels=labels).backward()
    deep_sink, wide_sink = _sinks(model)
    (d_ids, d_grad), = [(i.clone(), g.clone()) for i, g in deep_sink]
    (w_ids, w_grad), = [(i.clone(), g.clone()) for i, g in wide_sink]
    dt, ds, wt, ws = [t.detach().clone() for t in _tables(model)]
    model.apply_sparse_updates(LR)
    ops.emb_bwd_adagrad(dt, ds, d_ids, d_grad.reshape(d_ids.numel(), -1),
                        lr=LR)
    ops.emb_bwd_adagrad_wide(wt, ws, w_ids, w_grad, lr=LR)
    for got, want in zip(_tables(model), (dt, ds, wt, ws)):
        assert torch.allclose(got.detach(), want, atol=1e-6)
    assert not deep_sink and not wide_sink


@pytest.mark.parametrize("sharded", [False, True])
def test_model_applies_the_reference_op_and_carries_state(sharded):
    torch.manual_seed(5)
    model = _model(sharded=sharded)
    _step_and_check(model, seed=10)
    state_after_1 = _tables(model)[1].clone()
    assert state_after_1.abs().sum() > 0
    # the second step's reference starts from the first step's state
    _step_and_check(model, seed=11)
    assert (_tables(model)[1] >= state_after_1).all()
    assert not torch.equal(_tables(model)[1], state_after_1)


def test_sharded_world1_agrees_with_replicated():
    torch.manual_seed(6)
    rep = _model()
    sh = _model(sharded=True)
    sh.embeddings.weight.data.copy_(rep.deep_embedding.weight.data)
    sh.embeddings.wide_weight.data.copy_(rep.wide_embedding.weight.data)
    for name in ("wide_dense", "mlp", "head"):
        getattr(sh, name).load_state_dict(getattr(rep, name).state_dict())
    for seed in (20, 21):
        dense, ids, labels = _batch(seed)
        for m in (rep, sh):
            m(dense, ids, labels=labels).backward()
            m.apply_sparse_updates(LR)
    for a, b in zip(_tables(rep), _tables(sh)):
        assert torch.allclose(a.detach(), b.detach(), atol=1e-6)


@pytest.mark.parametrize("sharded", [False, True])
def test_state_dict_round_trip_carries_the_accumulator(sharded):
    torch.manual_seed(7)
    model = _model(sharded=sharded)
    for seed in (30, 31):
        dense, ids, labels = _batch(seed)
        model(dense, ids, labels=labels).backward()
        model.apply_sparse_updates(LR)
    sd = copy.deepcopy(model.state_dict())
    assert any(k.endswith("state_sum") for k in sd)
    assert not any("_adagrad" in k for k in sd)  # scratch is not saved
    fresh = _model(sharded=sharded)
    fresh.load_state_dict(sd)
    dense, ids, labels = _batch(32)
    for m in (model, fresh):
        m(dense, ids, labels=labels).backward()
        m.apply_sparse_updates(LR)
    for a, b in zip(_tables(model), _tables(fresh)):
        assert torch.equal(a.detach(), b.detach())


def test_initial_accumulator_and_eps_reach_the_update():
    torch.manual_seed(8)
    emb = SparseEmbedding([20], 4, sparse_optimizer="adagrad",
                          sparse_eps=1e-3, sparse_initial_accumulator=0.1)
    assert torch.equal(emb.state_sum, torch.full((20, 4), 0.1))
    t, s = emb.weight.detach().clone(), emb.state_sum.clone()
    ids = torch.randint(0, 20, (8, 1))
    g = torch.randn(8, 4)
    emb(ids).backward(g)
    emb.apply_sparse_updates(LR)
    ops.emb_bwd_adagrad(t, s, ids, g, lr=LR, eps=1e-3)
    assert torch.allclose(emb.weight.detach(), t, atol=1e-6)
    assert torch.allclose(emb.state_sum, s, atol=1e-6)


def test_pickle_and_deepcopy_drop_the_scratch_but_keep_training():
    import pickle
    torch.manual_seed(9)
    model = _model(sharded=True)
    dense, ids, labels = _batch(50)
    model(dense, ids, labels=labels).backward()
    model.apply_sparse_updates(LR)
    assert model.embeddings._adagrad_acc is not None
    clones = [copy.deepcopy(model), pickle.loads(pickle.dumps(model))]
    for c in clones:
        assert c.embeddings._adagrad_acc is None
        assert c.embeddings._adagrad_stamp is None
        assert torch.equal(c.embeddings.state_sum,
                           model.embeddings.state_sum)
    dense, ids, labels = _batch(51)
    for m in [model] + clones:
        m(dense, ids, labels=labels).backward()
        m.apply_sparse_updates(LR)
    for c in clones:
        for a, b in zip(_tables(model), _tables(c)):
            assert torch.equal(a.detach(), b.detach())


def test_default_model_is_unchanged():
    plain = WideAndDeep(table_sizes=TABLES, embedding_dim=4, hidden=(8,))
    sgd = WideAndDeep(table_sizes=TABLES, embedding_dim=4, hidden=(8,),
                      sparse_optimizer="sgd")
    assert list(sgd.state_dict().keys()) == list(plain.state_dict().keys())
    assert not any("state_sum" in k for k in plain.state_dict())
    assert [n for n, _ in sgd.named_buffers()] == \
        [n for n, _ in plain.named_buffers()]
    for sharded in (False, True):
        a = WideAndDeep(table_sizes=TABLES, embedding_dim=4, hidden=(8,),
                        sharded=sharded, sparse_optimizer="sgd")
        b = WideAndDeep(table_sizes=TABLES, embedding_dim=4, hidden=(8,),
                        sharded=sharded)
        assert list(a.state_dict().keys()) == list(b.state_dict().keys())
    flat = FlatInputWideAndDeep(table_sizes=TABLES, embedding_dim=4,
                                hidden=(8,), sparse_optimizer="adagrad")
    assert "net.deep_embedding.state_sum" in flat.state_dict()
    with pytest.raises(ValueError):
        WideScalarEmbedding(TABLES, sparse_optimizer="adam")


def test_adagrad_buffers_are_never_rebroadcast():
    """BucketedDataParallel re-broadcasts every unflagged buffer per
    forward; the table-sized Adagrad buffers must all carry the flag,
    also after a device/dtype move and after the first apply."""
    for sharded in (False, True):
        model = _model(sharded=sharded)
        dense, ids, labels = _batch(40)
        model(dense, ids, labels=labels).backward()
        model.apply_sparse_updates(LR)
        model = model.double()  # _apply replaces every float buffer
        big = [(n, b) for n, b in model.named_buffers()
               if "state_sum" in n or "_adagrad" in n]
        assert len(big) >= 5
        for n, b in big:
            assert getattr(b, "_miyarn_sharded", False), n


# ---- 2-rank gloo, feature-sharded ------------------------------------------

F, D, ROWS, B, W = 4, 8, 50, 6, 2
G_TABLES = [ROWS] * F
G_LR = 0.25
STEPS = 2


def _global_tables(seed=123):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(ROWS * F, D, generator=g),
            torch.randn(ROWS * F, 1, generator=g) * 0.01)


def _global_batch(step):
    g = torch.Generator().manual_seed(7 + step)
    return torch.randint(0, 10, (W * B, F), generator=g)


def _shard_rows(table, rank):
    return torch.cat([table[f * ROWS:(f + 1) * ROWS] for f in range(F)
                      if f % W == rank])


def _single_process_reference():
    """Full tables, global-mean loss, dense Adagrad (zero-gradient rows
    do not move, so dense == coalesced sparse)."""
    deep, wide = _global_tables()
    sd, sw = torch.zeros_like(deep), torch.zeros_like(wide)
    offs = torch.arange(F) * ROWS
    for step in range(STEPS):
        deep.requires_grad_(True)
        wide.requires_grad_(True)
        flat = (_global_batch(step) + offs).reshape(-1)
        out = deep.index_select(0, flat).reshape(W * B, F * D)
        wide_out = wide.reshape(-1).index_select(0, flat).reshape(
            W * B, F).sum(dim=1)
        (out.pow(2).mean() + wide_out.pow(2).mean()).backward()
        new = []
        for t, s in ((deep, sd), (wide, sw)):
            g = t.grad
            s += g * g
            new.append(t.detach() - G_LR * g / (s.sqrt() + 1e-10))
        deep, wide = new
    return deep, wide, sd, sw


def _gloo_worker(rank, kv_addr, out_q):
    from tf_yarn_amd.models.sharded_embedding import \
        ShardedCriteoEmbeddings
    from tf_yarn_amd.parallel import comm
    client = KVClient(kv_addr)
    comm.init_process_group(rank=rank, world_size=W, backend="gloo",
                            kv_client=client)
    try:
        emb = ShardedCriteoEmbeddings(G_TABLES, D,
                                      sparse_optimizer="adagrad")
        deep, wide = _global_tables()
        emb.weight.data.copy_(_shard_rows(deep, rank))
        emb.wide_weight.data.copy_(_shard_rows(wide, rank))
        for step in range(STEPS):
            ids = _global_batch(step)[rank * B:(rank + 1) * B]
            out_buf, wide_out = emb(ids, torch.zeros(B, F * D), 0)
            (out_buf.pow(2).mean() + wide_out.pow(2).mean()).backward()
            emb.apply_sparse_updates(G_LR)
        out_q.put((rank,) + tuple(
            t.detach().numpy().copy()
            for t in (emb.weight, emb.wide_weight, emb.state_sum,
                      emb.wide_state_sum)))
    finally:
        comm.destroy_process_group()


@pytest.mark.timeout(180)
def test_sharded_adagrad_two_ranks_matches_single_process():
    server = KVServer()
    ctx = mp.get_context("spawn")
    out_q = ctx.Queue()
    procs = [ctx.Process(target=_gloo_worker,
                         args=(r, server.address, out_q))
             for r in range(W)]
    for p in procs:
        p.start()
    try:
        results = {}
        for _ in range(W):
            got = out_q.get(timeout=150)
            results[got[0]] = [torch.from_numpy(a) for a in got[1:]]
    finally:
        for p in procs:
            p.join(timeout=30)
            if p.is_alive():
                p.terminate()
        server.stop()
    ref = _single_process_reference()
    names = ("deep", "wide", "deep state", "wide state")
    for r in range(W):
        for got, want, name in zip(results[r], ref, names):
            assert torch.allclose(got, _shard_rows(want, r), atol=1e-5), \
                f"rank {r} {name} mismatch"
