"""Sparse FTRL-proximal for the embedding tables and the per-table rule
choice: the CPU ops against an independent float64 evaluation of the
rule, lazy semantics, exact zeros under L1, the model wiring (replicated,
sharded, checkpoints, 2-rank gloo) and the dense ``FusedFtrl``.

The rule (TF ``Ftrl``, ``learning_rate_power=-0.5``, no beta, no L2
shrinkage), per element, G the summed and scaled gradient of a unique id::

    n' = n + G*G
    z' = z + G - (sqrt(n') - sqrt(n)) / lr * w
    w' = (sign(z') * l1 - z') / (sqrt(n') / lr + 2*l2)   if |z'| > l1
         0.0                                              otherwise

Tolerance: ``torch.allclose(atol=1e-5)`` (rtol 1e-5), the project's own
for optimizer kernels.  The fp32 op deviates from the float64 loop by at
most 2.8e-7 in w, 7.7e-6 in z (|z| up to 53, so 5e-4 is allowed there) and
5e-8 relative in n at these shapes, so the bound sits well above fp32
rounding of the rule and far below any error of the rule itself."""

import copy
import math
import pickle

import pytest
import torch
import torch.multiprocessing as mp

from tf_yarn_amd import ops
from tf_yarn_amd.kv import KVClient, KVServer
from tf_yarn_amd.models.wide_deep import (SPARSE_OPTIMIZERS,
                                          FlatInputWideAndDeep,
                                          SparseEmbedding, WideAndDeep,
                                          WideScalarEmbedding)

LR = 0.05
# elements this close to the |z'| == l1 threshold may fall on either side
# in fp32; the weight is continuous through 0 there
Z_MARGIN = 1e-4


def _close(got, want):
    return torch.allclose(got.double(), want, atol=1e-5, rtol=1e-5)


def _ftrl_loop64(w, n, z, ids, rows, lr, l1, l2, scale):
    """Independent evaluation: float64, one Python iteration per unique
    id, straight from the formulas.  Updates w, n, z (float64) in place
    and returns {id: z'} of the touched rows."""
    flat = ids.reshape(-1)
    rows = rows.double()
    z_new = {}
    for u in sorted(set(flat.tolist())):
        g = scale * rows[flat == u].sum(dim=0)
        n1 = n[u] + g * g
        z1 = z[u] + g - (n1.sqrt() - n[u].sqrt()) / lr * w[u]
        q = n1.sqrt() / lr + 2.0 * l2
        w1 = torch.zeros_like(z1)
        big = z1.abs() > l1
        w1[big] = (torch.sign(z1[big]) * l1 - z1[big]) / q[big]
        w[u], n[u], z[u] = w1, n1, z1
        z_new[u] = z1
    return z_new


def _exact_grads(gen, shape):
    return torch.randint(-32, 33, shape, generator=gen).float() / 8


# ---- reference ops vs the float64 loop --------------------------------------

@pytest.mark.parametrize("l1,l2", [(0.0, 0.0), (0.5, 0.25)])
@pytest.mark.parametrize("dim", [16, 1])
def test_op_matches_float64_loop(dim, l1, l2):
    gen = torch.Generator().manual_seed(dim + int(l1 * 10))
    rows, n_ids, scale = 60, 200, 0.5
    w = torch.randn(rows, dim, generator=gen)
    n = torch.full((rows, dim), 0.1)
    z = torch.zeros(rows, dim)
    w64, n64, z64 = w.double(), n.double(), z.double()
    for step in range(3):
        ids = torch.randint(0, 40, (n_ids,), generator=gen)  # duplicates
        grad = _exact_grads(gen, (n_ids, dim))
        ops.emb_bwd_ftrl(w, n, z, ids, grad, lr=LR, l1=l1, l2=l2,
                         scale=scale)
        _ftrl_loop64(w64, n64, z64, ids, grad, LR, l1, l2, scale)
        assert _close(w, w64) and _close(n, n64) and _close(z, z64), step


@pytest.mark.parametrize("l1,l2", [(0.0, 0.0), (0.5, 0.25)])
def test_wide_op_matches_float64_loop(l1, l2):
    gen = torch.Generator().manual_seed(11)
    rows, b, f, scale = 60, 32, 4, 0.5
    w = torch.randn(rows, 1, generator=gen)
    n = torch.full((rows, 1), 0.1)
    z = torch.zeros(rows, 1)
    w64, n64, z64 = w.double(), n.double(), z.double()
    for step in range(3):
        ids = torch.randint(0, 40, (b, f), generator=gen)
        gw = _exact_grads(gen, (b,))
        ops.emb_bwd_ftrl_wide(w, n, z, ids, gw, lr=LR, l1=l1, l2=l2,
                              scale=scale)
        per_update = gw.reshape(-1, 1).expand(-1, f).reshape(-1, 1)
        _ftrl_loop64(w64, n64, z64, ids, per_update, LR, l1, l2, scale)
        assert _close(w, w64) and _close(n, n64) and _close(z, z64), step


def test_untouched_rows_are_bit_identical_and_zero_sum_rows_move():
    gen = torch.Generator().manual_seed(3)
    w = torch.randn(100, 16, generator=gen)
    n = torch.rand(100, 16, generator=gen) + 0.1
    z = torch.randn(100, 16, generator=gen) * 0.1
    w0, n0, z0 = w.clone(), n.clone(), z.clone()
    ids = torch.randint(1, 50, (200,), generator=gen) * 2  # even rows, not 0
    grad = _exact_grads(gen, (200, 16))
    # row 0 gets +g and -g: its gradient sums to exactly 0
    g = _exact_grads(gen, (1, 16))
    ids = torch.cat([ids, torch.tensor([0, 0])])
    grad = torch.cat([grad, g, -g])
    ops.emb_bwd_ftrl(w, n, z, ids, grad, lr=LR, l1=0.01, l2=0.0)
    odd = torch.arange(1, 100, 2)
    for got, start in ((w, w0), (n, n0), (z, z0)):
        assert torch.equal(got[odd], start[odd])
    # lazy, not dense: the zero-sum row keeps (n, z) and has its weight
    # recomputed from them
    assert torch.equal(n[0], n0[0]) and torch.equal(z[0], z0[0])
    q = n0[0].double().sqrt() / LR
    z00 = z0[0].double()
    want = torch.where(z00.abs() > 0.01,
                       (torch.sign(z00) * 0.01 - z00) / q,
                       torch.zeros_like(z00))
    assert _close(w[0], want)
    assert not torch.equal(w[0], w0[0])


@pytest.mark.parametrize("l1", [0.5, 4.0])
def test_l1_produces_exact_zeros(l1):
    gen = torch.Generator().manual_seed(17)
    rows, dim, n_ids, scale, l2 = 500, 16, 1000, 0.5, 0.25
    w = torch.randn(rows, dim, generator=gen)
    n = torch.full((rows, dim), 0.1)
    z = torch.zeros(rows, dim)
    w64, n64, z64 = w.double(), n.double(), z.double()
    touched = torch.zeros(rows, dtype=torch.bool)
    last_z = {}
    for _ in range(3):
        ids = torch.randint(0, rows, (n_ids,), generator=gen)
        grad = _exact_grads(gen, (n_ids, dim))
        ops.emb_bwd_ftrl(w, n, z, ids, grad, lr=LR, l1=l1, l2=l2,
                         scale=scale)
        last_z.update(_ftrl_loop64(w64, n64, z64, ids, grad, LR, l1, l2,
                                   scale))
        touched[ids] = True
    zero_share = float((w64[touched] == 0.0).double().mean())
    print(f"l1={l1}: {zero_share:.1%} of touched elements are exactly 0")
    if l1 == 4.0:
        # the case that must sit well inside the branch on both sides
        assert 0.10 <= zero_share <= 0.90
    assert zero_share > 0
    # same zero set in fp32, away from the threshold
    sure = torch.zeros(rows, dim, dtype=torch.bool)
    for u, zu in last_z.items():
        sure[u] = (zu.abs() - l1).abs() >= Z_MARGIN
    assert float((~sure[touched]).double().mean()) <= 0.01
    assert torch.equal((w == 0.0)[sure], (w64 == 0.0)[sure])
    assert _close(w, w64)


def test_fused_pair_ops_equal_the_single_table_ops_on_cpu():
    gen = torch.Generator().manual_seed(4)
    n_ids, f, dim = 96, 4, 16
    ids = torch.randint(0, 30, (n_ids,), generator=gen)
    grad = torch.randn(n_ids, dim, generator=gen)
    gw = torch.randn(n_ids // f, generator=gen)

    def fresh():
        g = torch.Generator().manual_seed(5)
        return (torch.randn(60, dim, generator=g),
                torch.full((60, dim), 0.1), torch.zeros(60, dim),
                torch.randn(60, 1, generator=g),
                torch.full((60, 1), 0.1), torch.zeros(60, 1))

    t, s, _, w, wn, wz = fresh()
    ops.emb_bwd_adagrad_ftrl_fused_wide(t, s, w, wn, wz, ids, grad, gw,
                                        lr=LR, wide_lr=0.5, l1=0.01,
                                        l2=0.02)
    t2, s2, _, w2, wn2, wz2 = fresh()
    ops.emb_bwd_adagrad(t2, s2, ids, grad, lr=LR)
    ops.emb_bwd_ftrl_wide(w2, wn2, wz2, ids, gw, lr=0.5, l1=0.01, l2=0.02)
    for a, b in ((t, t2), (s, s2), (w, w2), (wn, wn2), (wz, wz2)):
        assert torch.equal(a, b)

    t, n, z, w, wn, wz = fresh()
    ops.emb_bwd_ftrl_fused_wide(t, n, z, w, wn, wz, ids, grad, gw, lr=LR,
                                l1=0.01, l2=0.02)  # wide_lr defaults to lr
    t2, n2, z2, w2, wn2, wz2 = fresh()
    ops.emb_bwd_ftrl(t2, n2, z2, ids, grad, lr=LR, l1=0.01, l2=0.02)
    ops.emb_bwd_ftrl_wide(w2, wn2, wz2, ids, gw, lr=LR, l1=0.01, l2=0.02)
    for a, b in ((t, t2), (n, n2), (z, z2), (w, w2), (wn, wn2), (wz, wz2)):
        assert torch.equal(a, b)


def test_bad_arguments_raise_on_cpu_and_change_nothing():
    w, n, z = torch.randn(10, 4), torch.ones(10, 4), torch.zeros(10, 4)
    w0 = w.clone()
    ids, grad = torch.arange(5), torch.ones(5, 4)
    for kw in (dict(lr=0.0), dict(lr=-1.0), dict(lr=LR, l1=-0.1),
               dict(lr=LR, l2=-0.1)):
        with pytest.raises(ValueError):
            ops.emb_bwd_ftrl(w, n, z, ids, grad, **kw)
        with pytest.raises(ValueError):
            ops.fused_ftrl(w.view(-1), torch.ones(40), n.view(-1),
                           z.view(-1), **kw)
    assert torch.equal(w, w0) and not z.any()
    assert ops.SparseWorkspace is ops.SparseAdagradWorkspace


# ---- model wiring -----------------------------------------------------------

TABLES = [50] * 4
L1, L2, WIDE_LR = 0.002, 0.01, 0.3
RECIPE = dict(sparse_optimizer="adagrad", wide_sparse_optimizer="ftrl",
              sparse_l1=L1, sparse_l2=L2, wide_sparse_lr=WIDE_LR,
              sparse_initial_accumulator=0.1)


def _model(**kw):
    return WideAndDeep(table_sizes=TABLES, embedding_dim=4, hidden=(8,),
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


def _sparse_tensors(model):
    """Every table and rule state of the model, by state_dict key."""
    return {k: v for k, v in model.state_dict().items()
            if "embedding" in k and "offsets" not in k}


def _state_keys(model):
    return sorted(k.split(".", 1)[1] for k in model.state_dict()
                  if "state_sum" in k or "ftrl" in k)


def test_ftrl_is_an_accepted_rule_and_others_still_raise():
    assert SPARSE_OPTIMIZERS == ("sgd", "adagrad", "ftrl")
    with pytest.raises(ValueError):
        _model(sparse_optimizer="adam")
    with pytest.raises(ValueError):
        _model(wide_sparse_optimizer="adam")
    with pytest.raises(ValueError):
        _model(sparse_optimizer="ftrl", sparse_l1=-1.0)
    with pytest.raises(ValueError):
        WideScalarEmbedding(TABLES, sparse_optimizer="ftrl",
                            sparse_l2=-1.0)


@pytest.mark.parametrize("sharded", [False, True])
def test_state_dict_keys_per_rule_pair(sharded):
    def keys(**kw):
        return _state_keys(_model(sharded=sharded, **kw))

    wide = (lambda s: "wide_" + s) if sharded else (lambda s: s)
    assert keys() == []
    assert keys(sparse_optimizer="adagrad") == \
        sorted(["state_sum", wide("state_sum")])
    # a table owns state for its own rule only
    assert keys(sparse_optimizer="adagrad", wide_sparse_optimizer="ftrl") \
        == sorted(["state_sum", wide("ftrl_accum"), wide("ftrl_linear")])
    assert keys(sparse_optimizer="ftrl") == sorted(
        ["ftrl_accum", "ftrl_linear", wide("ftrl_accum"),
         wide("ftrl_linear")])
    assert keys(wide_sparse_optimizer="ftrl") == \
        sorted([wide("ftrl_accum"), wide("ftrl_linear")])
    assert keys(sparse_optimizer="ftrl", wide_sparse_optimizer="sgd") == \
        ["ftrl_accum", "ftrl_linear"]
    m = _model(sharded=sharded, **RECIPE)
    sd = m.state_dict()
    prefix = "embeddings.wide_" if sharded else "wide_embedding."
    assert prefix + "state_sum" not in sd
    assert torch.equal(sd[prefix + "ftrl_accum"],
                       torch.full((sum(TABLES), 1), 0.1))
    assert not sd[prefix + "ftrl_linear"].any()
    assert sd[prefix + "ftrl_accum"].dtype == torch.float32
    flat = FlatInputWideAndDeep(table_sizes=TABLES, embedding_dim=4,
                                hidden=(8,), **RECIPE)
    assert "net.wide_embedding.ftrl_linear" in flat.state_dict()


def test_sgd_and_adagrad_models_keep_their_keys_and_buffers():
    base = ["deep_embedding.offsets", "wide_embedding.offsets"]
    sharded_base = ["embeddings.own_offsets", "embeddings.full_offsets",
                    "embeddings.own_offsets_tiled"]
    for kw in (dict(), dict(sparse_optimizer="sgd")):
        assert [n for n, _ in _model(**kw).named_buffers()] == base
        assert [n for n, _ in _model(sharded=True, **kw).named_buffers()] \
            == sharded_base
    ada = _model(sparse_optimizer="adagrad")
    assert [n for n, _ in ada.named_buffers()] == [
        "deep_embedding.offsets", "deep_embedding.state_sum",
        "wide_embedding.offsets", "wide_embedding.state_sum"]
    ada_sh = _model(sparse_optimizer="adagrad", sharded=True)
    assert [n for n, _ in ada_sh.named_buffers()] == [
        "embeddings.state_sum", "embeddings.wide_state_sum"] + sharded_base
    assert [k for k in ada_sh.state_dict() if k.startswith("embeddings")] \
        == ["embeddings.weight", "embeddings.wide_weight",
            "embeddings.state_sum", "embeddings.wide_state_sum",
            "embeddings.own_offsets", "embeddings.full_offsets"]
    _train(ada_sh, (1,))
    e = ada_sh.embeddings
    assert e._adagrad_acc is not None and e._adagrad_acc1 is not None
    assert e._adagrad_stamp is not None
    assert ada_sh.wide_sparse_optimizer == "adagrad"


@pytest.mark.parametrize("sharded", [False, True])
def test_recipe_model_applies_the_reference_ops(sharded):
    torch.manual_seed(5)
    model = _model(sharded=sharded, **RECIPE)
    if sharded:
        e = model.embeddings
        got = (e.weight, e.state_sum, e.wide_weight, e.wide_ftrl_accum,
               e.wide_ftrl_linear)
        sinks = (e._deep_sink, e._wide_sink)
    else:
        d, w = model.deep_embedding, model.wide_embedding
        got = (d.weight, d.state_sum, w.weight, w.ftrl_accum,
               w.ftrl_linear)
        sinks = (d.pending_grads(), w.pending_grads())
    for seed in (10, 11):
        dense, ids, labels = _batch(seed)
        model(dense, ids, labels=labels).backward()
        (d_ids, d_grad), = [(i.clone(), g.clone()) for i, g in sinks[0]]
        (w_ids, w_grad), = [(i.clone(), g.clone()) for i, g in sinks[1]]
        dt, ds, wt, wn, wz = [t.detach().clone() for t in got]
        model.apply_sparse_updates(LR)
        ops.emb_bwd_adagrad(dt, ds, d_ids,
                            d_grad.reshape(d_ids.numel(), -1), lr=LR)
        # wide_sparse_lr, sparse_l1 and sparse_l2 reach the update
        ops.emb_bwd_ftrl_wide(wt, wn, wz, w_ids, w_grad, lr=WIDE_LR,
                              l1=L1, l2=L2)
        for a, b in zip(got, (dt, ds, wt, wn, wz)):
            assert torch.allclose(a.detach(), b, atol=1e-6)
        assert not sinks[0] and not sinks[1]
    assert got[4].abs().sum() > 0
    # different knobs give a different table
    other = torch.zeros_like(wt)
    ops.emb_bwd_ftrl_wide(other, wn.clone(), wz.clone(), w_ids, w_grad,
                          lr=LR, l1=0.0, l2=0.0)
    assert not torch.allclose(other, wt, atol=1e-6)


def test_sharded_world1_agrees_with_replicated():
    for kw in (RECIPE, dict(sparse_optimizer="ftrl", sparse_l1=L1),
               dict(sparse_optimizer="ftrl", wide_sparse_optimizer="adagrad"),
               dict(wide_sparse_optimizer="ftrl", wide_sparse_lr=WIDE_LR)):
        torch.manual_seed(6)
        rep = _model(**kw)
        sh = _model(sharded=True, **kw)
        sh.embeddings.weight.data.copy_(rep.deep_embedding.weight.data)
        sh.embeddings.wide_weight.data.copy_(
            rep.wide_embedding.weight.data)
        for name in ("wide_dense", "mlp", "head"):
            getattr(sh, name).load_state_dict(
                getattr(rep, name).state_dict())
        _train(rep, (20, 21))
        _train(sh, (20, 21))
        assert torch.allclose(sh.embeddings.weight,
                              rep.deep_embedding.weight, atol=1e-6)
        assert torch.allclose(sh.embeddings.wide_weight,
                              rep.wide_embedding.weight, atol=1e-6)


@pytest.mark.parametrize("sharded", [False, True])
@pytest.mark.parametrize("deep_rule", ["adagrad", "ftrl"])
def test_checkpoint_round_trip_then_one_more_step(deep_rule, sharded):
    torch.manual_seed(7)
    kw = dict(RECIPE, sparse_optimizer=deep_rule, sharded=sharded)
    model = _model(**kw)
    _train(model, (30, 31))
    sd = copy.deepcopy(model.state_dict())
    assert any(k.endswith("ftrl_linear") for k in sd)
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
    model = _model(sharded=sharded, **RECIPE)
    _train(model, (50,))
    owners = ([model.embeddings] if sharded
              else [model.deep_embedding, model.wide_embedding])
    assert all(o._adagrad_acc is not None for o in owners)
    clones = [copy.deepcopy(model), pickle.loads(pickle.dumps(model))]
    for c in clones:
        c_owners = ([c.embeddings] if sharded
                    else [c.deep_embedding, c.wide_embedding])
        for o in c_owners:
            assert o._adagrad_acc is None and o._adagrad_stamp is None
            assert o._sparse_ws is None
        if sharded:
            assert c.embeddings._adagrad_acc1 is None
    _train(model, (51,))
    ref = _sparse_tensors(model)
    for c in clones:
        _train(c, (51,))
        for k, v in _sparse_tensors(c).items():
            assert torch.equal(v, ref[k]), k


def test_table_sized_buffers_stay_flagged_after_double():
    for sharded in (False, True):
        for kw in (RECIPE, dict(sparse_optimizer="ftrl")):
            model = _model(sharded=sharded, **kw)
            _train(model, (40,))
            model = model.double()  # _apply replaces every float buffer
            big = [(n, b) for n, b in model.named_buffers()
                   if "state_sum" in n or "ftrl" in n or "_adagrad" in n]
            assert len(big) >= 6
            for n, b in big:
                assert getattr(b, "_miyarn_sharded", False), n


def test_single_table_modules_take_the_ftrl_arguments():
    torch.manual_seed(8)
    emb = SparseEmbedding([20], 4, sparse_optimizer="ftrl", sparse_l1=0.01,
                          sparse_l2=0.02, sparse_initial_accumulator=0.1)
    assert torch.equal(emb.ftrl_accum, torch.full((20, 4), 0.1))
    t, n, z = (emb.weight.detach().clone(), emb.ftrl_accum.clone(),
               emb.ftrl_linear.clone())
    ids = torch.randint(0, 20, (8, 1))
    g = torch.randn(8, 4)
    emb(ids).backward(g)
    emb.apply_sparse_updates(LR)
    ops.emb_bwd_ftrl(t, n, z, ids, g, lr=LR, l1=0.01, l2=0.02)
    assert torch.equal(emb.weight.detach(), t)
    assert torch.equal(emb.ftrl_accum, n)
    assert torch.equal(emb.ftrl_linear, z)


# ---- 2-rank gloo, feature-sharded, Adagrad deep + FTRL wide -----------------

F, D, ROWS, B, W = 4, 8, 50, 6, 2
G_TABLES = [ROWS] * F
G_LR, G_WIDE_LR, G_L1, G_L2, G_INIT = 0.25, 0.5, 0.0005, 0.01, 0.1
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
    """Full tables, global-mean loss.  Deep: dense Adagrad (zero-gradient
    rows do not move, so dense == coalesced sparse).  Wide: FTRL on the
    batch's unique rows ONLY — a dense FTRL step would recompute, and so
    wipe, the weights of rows the batch never named."""
    deep, wide = _global_tables()
    sd = torch.full_like(deep, G_INIT)
    wn, wz = torch.full_like(wide, G_INIT), torch.zeros_like(wide)
    offs = torch.arange(F) * ROWS
    for step in range(STEPS):
        deep.requires_grad_(True)
        wide.requires_grad_(True)
        flat = (_global_batch(step) + offs).reshape(-1)
        out = deep.index_select(0, flat).reshape(W * B, F * D)
        wide_out = wide.reshape(-1).index_select(0, flat).reshape(
            W * B, F).sum(dim=1)
        (out.pow(2).mean() + wide_out.pow(2).mean()).backward()
        g = deep.grad
        sd += g * g
        deep = deep.detach() - G_LR * g / (sd.sqrt() + 1e-10)
        u = torch.unique(flat)
        g, w = wide.grad[u], wide.detach()[u]
        n1 = wn[u] + g * g
        z1 = wz[u] + g - (n1.sqrt() - wn[u].sqrt()) / G_WIDE_LR * w
        q = n1.sqrt() / G_WIDE_LR + 2 * G_L2
        w1 = torch.where(z1.abs() > G_L1,
                         (torch.sign(z1) * G_L1 - z1) / q,
                         torch.zeros_like(z1))
        wide = wide.detach().clone()
        wide[u], wn[u], wz[u] = w1, n1, z1
    return deep, wide, sd, wn, wz


def _gloo_worker(rank, kv_addr, out_q):
    from tf_yarn_amd.models.sharded_embedding import \
        ShardedCriteoEmbeddings
    from tf_yarn_amd.parallel import comm
    client = KVClient(kv_addr)
    comm.init_process_group(rank=rank, world_size=W, backend="gloo",
                            kv_client=client)
    try:
        emb = ShardedCriteoEmbeddings(
            G_TABLES, D, sparse_optimizer="adagrad",
            wide_sparse_optimizer="ftrl", sparse_l1=G_L1, sparse_l2=G_L2,
            wide_sparse_lr=G_WIDE_LR, sparse_initial_accumulator=G_INIT)
        deep, wide = _global_tables()
        emb.weight.data.copy_(_shard_rows(deep, rank))
        emb.wide_weight.data.copy_(_shard_rows(wide, rank))
        for step in range(STEPS):
            ids = _global_batch(step)[rank * B:(rank + 1) * B]
            out_buf, wide_out = emb(ids, torch.zeros(B, F * D), 0)
            (out_buf.pow(2).mean() + wide_out.pow(2).mean()).backward()
            emb.apply_sparse_updates(G_LR)
        assert not hasattr(emb, "wide_state_sum")
        out_q.put((rank,) + tuple(
            t.detach().numpy().copy()
            for t in (emb.weight, emb.wide_weight, emb.state_sum,
                      emb.wide_ftrl_accum, emb.wide_ftrl_linear)))
    finally:
        comm.destroy_process_group()


@pytest.mark.timeout(180)
def test_sharded_adagrad_ftrl_two_ranks_matches_single_process():
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
    names = ("deep", "wide", "deep state", "wide accum", "wide linear")
    for r in range(W):
        for got, want, name in zip(results[r], ref, names):
            assert torch.allclose(got, _shard_rows(want, r), atol=1e-5), \
                f"rank {r} {name} mismatch"
    # untouched wide rows kept their initial weights (lazy FTRL)
    _, wide0 = _global_tables()
    assert (ref[1] == wide0).double().mean() > 0.5


# ---- dense FTRL -------------------------------------------------------------

def test_fused_ftrl_optimizer_matches_float64_loop():
    from tf_yarn_amd.ops.optim import FusedFtrl
    torch.manual_seed(12)
    p = torch.nn.Parameter(torch.randn(37))
    skipped = torch.nn.Parameter(torch.randn(5))
    skipped._miyarn_sparse = True
    opt = FusedFtrl([p, skipped], lr=0.05, l1=0.05, l2=0.1)
    assert FusedFtrl([p]).defaults["lr"] == 0.001
    assert FusedFtrl([p]).defaults["initial_accumulator_value"] == 0.1
    w = p.detach().double().tolist()
    n, z = [0.1] * 37, [0.0] * 37
    skipped0 = skipped.detach().clone()
    for _ in range(3):
        p.grad = torch.randn(37)
        skipped.grad = torch.ones(5)
        opt.step()
        for i, g in enumerate(p.grad.double().tolist()):
            n1 = n[i] + g * g
            z[i] += g - (math.sqrt(n1) - math.sqrt(n[i])) / 0.05 * w[i]
            n[i] = n1
            q = math.sqrt(n1) / 0.05 + 2 * 0.1
            w[i] = ((math.copysign(0.05, z[i]) - z[i]) / q
                    if abs(z[i]) > 0.05 else 0.0)
        assert _close(p.detach(), torch.tensor(w, dtype=torch.float64))
    assert _close(opt.state[p]["accum"], torch.tensor(n, dtype=torch.float64))
    assert _close(opt.state[p]["linear"],
                  torch.tensor(z, dtype=torch.float64))
    assert torch.equal(skipped.detach(), skipped0)


def test_fused_ftrl_bf16_param_keeps_an_fp32_master():
    from tf_yarn_amd.ops.optim import FusedFtrl
    torch.manual_seed(13)
    p = torch.nn.Parameter(torch.randn(16).to(torch.bfloat16))
    opt = FusedFtrl([p], lr=0.05)
    p.grad = torch.randn(16).to(torch.bfloat16)
    opt.step()
    master = opt.state[p]["master"]
    assert master.dtype == torch.float32
    assert torch.equal(p.detach(), master.to(torch.bfloat16))


def test_ftrl_string_resolves_in_the_keras_shim_and_ps_step():
    from tf_yarn_amd.estimator.keras import _resolve_optimizer
    from tf_yarn_amd.ops.optim import FusedFtrl
    from tf_yarn_amd.parallel.ps import make_ftrl_step
    lin = torch.nn.Linear(3, 1)
    opt = _resolve_optimizer("ftrl", lin.parameters())
    assert isinstance(opt, FusedFtrl)
    assert opt.defaults["lr"] == 0.001
    shard, grad = torch.randn(9), torch.randn(9)
    w, n, z = shard.clone(), torch.full((9,), 0.1), torch.zeros(9)
    step = make_ftrl_step(0.05, l1=0.01)
    step(shard, grad)
    ops.fused_ftrl(w, grad, n, z, lr=0.05, l1=0.01)
    assert torch.equal(shard, w)
