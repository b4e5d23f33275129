"""Row-wise sparse Adagrad: the CPU op against an independent float64
evaluation of the rule, and the model wiring (replicated, sharded,
checkpoints, the rule names each table accepts).

The rule, per unique id u, G the summed and scaled gradient row::

    m             = (sum_c G[u, c]^2) / dim
    state_row[u] += m
    table[u, :]  -= lr * G[u, :] / (sqrt(state_row[u]) + eps)   (new state)

Tolerance against the float64 loop: ``torch.allclose(atol=1e-5,
rtol=1e-5)``, the project's own for optimizer kernels.  The fp32 op rounds
a sum of at most 16 squares, one division, one square root and one
division per element; with |G| <= 6 (state up to ~40 per step) that is a
few ulp of fp32, about 1e-6 relative, well inside the bound."""

import copy
import pickle

import pytest
import torch

from tf_yarn_amd import ops
from tf_yarn_amd.models import wide_deep
from tf_yarn_amd.models.wide_deep import (SPARSE_OPTIMIZERS,
                                          FlatInputWideAndDeep,
                                          SparseEmbedding, WideAndDeep,
                                          WideScalarEmbedding)

LR = 0.05
EPS = 1e-10


def _close(got, want):
    return torch.allclose(got.double(), want, atol=1e-5, rtol=1e-5)


def _rowwise_loop64(w, s, ids, rows, lr, eps, scale):
    """float64, one Python iteration per unique id, straight from the
    formula.  Updates w [rows, dim] and s [rows] (float64) in place."""
    flat = ids.reshape(-1)
    rows = rows.double()
    dim = w.shape[1]
    for u in sorted(set(flat.tolist())):
        g = scale * rows[flat == u].sum(dim=0)
        m = (g * g).sum() / dim
        s[u] = s[u] + m
        w[u] = w[u] - lr * g / (s[u].sqrt() + eps)


def _exact_grads(gen, shape, dtype=torch.float32):
    g = torch.randint(-32, 33, shape, generator=gen).float() / 8
    return g.to(dtype)


# ---- reference op vs the float64 loop ---------------------------------------

@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("dim", [16, 7, 1])
def test_op_matches_float64_loop(dim, dtype):
    gen = torch.Generator().manual_seed(dim)
    rows, n_ids, scale = 60, 200, 0.5
    w = torch.randn(rows, dim, generator=gen)
    s = torch.rand(rows, generator=gen)
    w0, s0 = w.clone(), s.clone()
    w64, s64 = w.double(), s.double()
    named = torch.zeros(rows, dtype=torch.bool)
    for step in range(3):
        ids = torch.randint(0, 40, (n_ids,), generator=gen)  # duplicates
        assert torch.unique(ids).numel() < n_ids
        grad = _exact_grads(gen, (n_ids, dim), dtype)
        ops.emb_bwd_rowwise_adagrad(w, s, ids, grad, lr=LR, eps=EPS,
                                    scale=scale)
        _rowwise_loop64(w64, s64, ids, grad, LR, EPS, scale)
        named[ids] = True
        assert _close(w, w64) and _close(s, s64), step
    assert s.shape == (rows,) and s.dtype == torch.float32
    assert named.any() and not named.all()
    assert torch.equal(w[~named], w0[~named])
    assert torch.equal(s[~named], s0[~named])
    assert not torch.equal(w[named], w0[named])


def test_dim1_is_elementwise_adagrad():
    gen = torch.Generator().manual_seed(2)
    w = torch.randn(50, 1, generator=gen)
    s = torch.rand(50, generator=gen)
    w2, s2 = w.clone(), s.clone().reshape(50, 1)
    ids = torch.randint(0, 30, (120,), generator=gen)
    grad = _exact_grads(gen, (120, 1))
    ops.emb_bwd_rowwise_adagrad(w, s, ids, grad, lr=LR, scale=0.5)
    ops.emb_bwd_adagrad(w2, s2, ids, grad, lr=LR, scale=0.5)
    assert torch.equal(w, w2) and torch.equal(s, s2.reshape(-1))


def test_fused_pair_ops_equal_the_single_table_ops_on_cpu():
    gen = torch.Generator().manual_seed(4)
    n_ids, f, dim = 96, 4, 16
    ids = torch.randint(0, 30, (n_ids,), generator=gen)
    grad = torch.randn(n_ids, dim, generator=gen)
    gw = torch.randn(n_ids // f, generator=gen)

    def fresh():
        g = torch.Generator().manual_seed(5)
        return (torch.randn(60, dim, generator=g), torch.full((60,), 0.1),
                torch.randn(60, 1, generator=g),
                torch.full((60, 1), 0.1), torch.zeros(60, 1))

    t, s, w, wn, wz = fresh()
    ops.emb_bwd_rowwise_adagrad_ftrl_fused_wide(
        t, s, w, wn, wz, ids, grad, gw, lr=LR, wide_lr=0.5, l1=0.01,
        l2=0.02)
    t2, s2, w2, wn2, wz2 = fresh()
    ops.emb_bwd_rowwise_adagrad(t2, s2, ids, grad, lr=LR)
    ops.emb_bwd_ftrl_wide(w2, wn2, wz2, ids, gw, lr=0.5, l1=0.01, l2=0.02)
    for a, b in ((t, t2), (s, s2), (w, w2), (wn, wn2), (wz, wz2)):
        assert torch.equal(a, b)

    t, s, w, ws_, _ = fresh()
    ops.emb_bwd_rowwise_adagrad_fused_wide(t, s, w, ws_, ids, grad, gw,
                                           lr=LR, scale=0.5)
    t2, s2, w2, ws2, _ = fresh()
    ops.emb_bwd_rowwise_adagrad(t2, s2, ids, grad, lr=LR, scale=0.5)
    ops.emb_bwd_adagrad_wide(w2, ws2, ids, gw, lr=LR, scale=0.5)
    for a, b in ((t, t2), (s, s2), (w, w2), (ws_, ws2)):
        assert torch.equal(a, b)
    with pytest.raises(ValueError):
        ops.emb_bwd_rowwise_adagrad_ftrl_fused_wide(
            t, s, w, wn, wz, ids, grad, gw, lr=LR, l1=-1.0)


# ---- model wiring -----------------------------------------------------------

TABLES = [50] * 4
ROWS = sum(TABLES)
DIM = 4
INIT = 0.1


def _model(**kw):
    kw.setdefault("sparse_optimizer", "rowwise_adagrad")
    kw.setdefault("sparse_initial_accumulator", INIT)
    return WideAndDeep(table_sizes=TABLES, embedding_dim=DIM, hidden=(8,),
                       **kw)


def _batch(seed, b=32):
    g = torch.Generator().manual_seed(seed)
    dense = torch.randn(b, 13, generator=g)
    ids = torch.randint(0, 12, (b, len(TABLES)), generator=g)
    labels = torch.rand(b, generator=g).round()
    return dense, ids, labels


def _train(model, seeds):
    for seed in seeds:
        dense, ids, labels = _batch(seed)
        model(dense, ids, labels=labels).backward()
        model.apply_sparse_updates(LR)


def _deep_owner(model):
    return model.embeddings if model.sharded else model.deep_embedding


def _sparse_tensors(model):
    return {k: v for k, v in model.state_dict().items()
            if "embedding" in k and "offsets" not in k}


def test_rule_names_per_table():
    assert SPARSE_OPTIMIZERS == ("sgd", "adagrad", "ftrl")
    assert wide_deep.DEEP_SPARSE_OPTIMIZERS == \
        SPARSE_OPTIMIZERS + ("rowwise_adagrad",)
    for sharded in (False, True):
        m = _model(sharded=sharded)
        assert m.sparse_optimizer == "rowwise_adagrad"
        # the wide table's default under a row-wise deep table
        assert m.wide_sparse_optimizer == "adagrad"
        wide_state = (m.embeddings.wide_state_sum if sharded
                      else m.wide_embedding.state_sum)
        assert wide_state.shape == (ROWS, 1)
        with pytest.raises(ValueError, match='"adagrad"'):
            _model(sharded=sharded,
                   wide_sparse_optimizer="rowwise_adagrad")
        with pytest.raises(ValueError, match='"adagrad"'):
            _model(sharded=sharded, sparse_optimizer="adagrad",
                   wide_sparse_optimizer="rowwise_adagrad")
        with pytest.raises(ValueError):
            _model(sharded=sharded, sparse_optimizer="rowwise_adam")
    with pytest.raises(ValueError, match='"adagrad"'):
        WideScalarEmbedding(TABLES, sparse_optimizer="rowwise_adagrad")
    emb = SparseEmbedding([20], 4, sparse_optimizer="rowwise_adagrad")
    assert emb.state_sum_row.shape == (20,)
    flat = FlatInputWideAndDeep(table_sizes=TABLES, embedding_dim=DIM,
                                hidden=(8,),
                                sparse_optimizer="rowwise_adagrad")
    assert "net.deep_embedding.state_sum_row" in flat.state_dict()
    assert flat.net.wide_sparse_optimizer == "adagrad"


@pytest.mark.parametrize("sharded", [False, True])
def test_model_owns_one_state_value_per_row(sharded):
    m = _model(sharded=sharded)
    e = _deep_owner(m)
    assert e.state_sum_row.numel() == ROWS
    assert e.state_sum_row.shape == (ROWS,)
    assert e.state_sum_row.dtype == torch.float32
    assert e.state_sum_row.is_contiguous()
    assert torch.equal(e.state_sum_row, torch.full((ROWS,), INIT))
    assert getattr(e.state_sum_row, "_miyarn_sharded", False)
    assert not hasattr(e, "state_sum")
    prefix = "embeddings." if sharded else "deep_embedding."
    sd = m.state_dict()
    assert prefix + "state_sum_row" in sd
    assert prefix + "state_sum" not in sd
    assert not any("ftrl" in k for k in sd)
    m = m.double().float()  # _apply replaces the buffer: the flag follows
    assert getattr(_deep_owner(m).state_sum_row, "_miyarn_sharded", False)


@pytest.mark.parametrize("wide_rule", ["adagrad", "ftrl", "sgd"])
@pytest.mark.parametrize("sharded", [False, True])
def test_model_applies_the_reference_ops(sharded, wide_rule):
    torch.manual_seed(5)
    l1, l2, wide_lr = 0.002, 0.01, 0.3
    model = _model(sharded=sharded, wide_sparse_optimizer=wide_rule,
                   sparse_l1=l1, sparse_l2=l2,
                   wide_sparse_lr=wide_lr if wide_rule != "adagrad"
                   else None)
    if sharded:
        e = model.embeddings
        deep_got = (e.weight, e.state_sum_row)
        wide_w, wp, wide_owner = e.wide_weight, "wide_", e
        sinks = (e._deep_sink, e._wide_sink)
    else:
        d, w = model.deep_embedding, model.wide_embedding
        deep_got = (d.weight, d.state_sum_row)
        wide_w, wp, wide_owner = w.weight, "", w
        sinks = (d.pending_grads(), w.pending_grads())
    wide_names = {"adagrad": ["state_sum"], "sgd": [],
                  "ftrl": ["ftrl_accum", "ftrl_linear"]}[wide_rule]
    wide_got = [wide_w] + [getattr(wide_owner, wp + n) for n in wide_names]
    for seed in (10, 11):
        dense, ids, labels = _batch(seed)
        model(dense, ids, labels=labels).backward()
        (d_ids, d_grad), = [(i.clone(), g.clone()) for i, g in sinks[0]]
        (w_ids, w_grad), = [(i.clone(), g.clone()) for i, g in sinks[1]]
        dt, ds = [t.detach().clone() for t in deep_got]
        wt = [t.detach().clone() for t in wide_got]
        model.apply_sparse_updates(LR)
        ops.emb_bwd_rowwise_adagrad(
            dt, ds, d_ids, d_grad.reshape(d_ids.numel(), -1), lr=LR)
        if wide_rule == "adagrad":
            ops.emb_bwd_adagrad_wide(*wt, w_ids, w_grad, lr=LR)
        elif wide_rule == "ftrl":
            ops.emb_bwd_ftrl_wide(*wt, w_ids, w_grad, lr=wide_lr, l1=l1,
                                  l2=l2)
        else:
            ops.emb_scatter_sum(wt[0],
                                w_ids.reshape(w_grad.numel(), -1), w_grad,
                                alpha=-wide_lr)
        for a, b in zip(list(deep_got) + wide_got, [dt, ds] + wt):
            assert torch.allclose(a.detach(), b, atol=1e-6)
        assert not sinks[0] and not sinks[1]
    assert (deep_got[1] != INIT).any() and (deep_got[1] == INIT).any()


def test_sharded_world1_agrees_with_replicated():
    torch.manual_seed(6)
    rep = _model()
    sh = _model(sharded=True)
    sh.embeddings.weight.data.copy_(rep.deep_embedding.weight.data)
    sh.embeddings.wide_weight.data.copy_(rep.wide_embedding.weight.data)
    for name in ("wide_dense", "mlp", "head"):
        getattr(sh, name).load_state_dict(getattr(rep, name).state_dict())
    _train(rep, (20, 21))
    _train(sh, (20, 21))
    assert torch.allclose(sh.embeddings.weight, rep.deep_embedding.weight,
                          atol=1e-6)
    assert torch.allclose(sh.embeddings.state_sum_row,
                          rep.deep_embedding.state_sum_row, atol=1e-6)
    assert torch.allclose(sh.embeddings.wide_weight,
                          rep.wide_embedding.weight, atol=1e-6)


@pytest.mark.parametrize("sharded", [False, True])
def test_checkpoint_round_trip_then_one_more_step(sharded):
    torch.manual_seed(7)
    kw = dict(sharded=sharded, wide_sparse_optimizer="ftrl",
              sparse_l1=0.002)
    model = _model(**kw)
    _train(model, (30, 31))
    sd = copy.deepcopy(model.state_dict())
    key, = [k for k in sd if k.endswith("state_sum_row")]
    assert sd[key].shape == (ROWS,) and (sd[key] != INIT).any()
    assert not any("_adagrad" in k for k in sd)  # scratch is not saved
    fresh = _model(**kw)
    fresh.load_state_dict(sd)
    _train(model, (32,))
    _train(fresh, (32,))
    a, b = _sparse_tensors(model), _sparse_tensors(fresh)
    assert len(a) >= 5
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("sharded", [False, True])
def test_pickle_and_deepcopy_drop_the_scratch_but_keep_training(sharded):
    torch.manual_seed(9)
    model = _model(sharded=sharded)
    _train(model, (50,))
    assert _deep_owner(model)._adagrad_acc is not None
    clones = [copy.deepcopy(model), pickle.loads(pickle.dumps(model))]
    for c in clones:
        o = _deep_owner(c)
        assert o._adagrad_acc is None and o._adagrad_stamp is None
        assert o._sparse_ws is None
        assert torch.equal(o.state_sum_row,
                           _deep_owner(model).state_sum_row)
    _train(model, (51,))
    ref = _sparse_tensors(model)
    for c in clones:
        _train(c, (51,))
        for k, v in _sparse_tensors(c).items():
            assert torch.equal(v, ref[k]), k
