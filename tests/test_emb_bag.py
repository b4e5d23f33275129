"""Multi-hot embedding bags on the CPU path: ``ops.emb_bag_fwd`` /
``ops.emb_bag_bwd_rows`` against a float64 loop, the module wiring against
a hand-expanded update, the host-side refusals, and two gloo ranks with
different ``nnz``.

Tolerance of the random-valued fp32 cases: the CPU path adds a bag's
``len`` terms one by one in fp32 (each add, or fma, rounds once: relative
2^-24 of the running sum, itself at most ``sum_i |w_i row_i|``).  The
denominator is such a sum of ``len`` positive terms (relative error at
most ``len * 2^-24``), its square root and reciprocal add 1.5 ulp, and
the final product rounds once more.  So ``|out - ref64| <= (2 len + 4) *
2^-24 * sum_i |w_i row_i| * |scale|``, the bound asserted below.  Integer-valued
operands make every sum exact, and those cases compare with
``torch.equal``."""

import copy

import pytest
import torch
import torch.multiprocessing as mp
import torch.nn.functional as F_

import emb_bag_ref as R
import exact_ints
from tf_yarn_amd import ops
from tf_yarn_amd.models.wide_deep import (BagUpdate, SparseEmbedding,
                                          WideAndDeep, _DeepInput)

SIZES = [7, 5, 6]          # rows per feature
NF = len(SIZES)
DIM = 4
# B = 4 examples x 3 features: empty bags first, in the middle and last, a
# long bag, and (rows are few) ids repeated inside bags
LENGTHS = [0, 3, 1, 2, 0, 5, 1, 1, 9, 2, 4, 0]
RULES = ("sgd", "adagrad", "rowwise_adagrad", "ftrl", "lazy_adam")


def _gen(seed=0):
    return torch.Generator().manual_seed(seed)


def _case(seed=0, lengths=LENGTHS, ints=False, weights=False):
    g = _gen(seed)
    ids, bo, offsets = R.make_bags(lengths, SIZES, g)
    rows = sum(SIZES)
    if ints:
        table = exact_ints.ints((rows, DIM), 8, g).float()
    else:
        table = torch.randn(rows, DIM, generator=g)
    w = None
    if weights:
        w = (torch.randint(-4, 5, (ids.numel(),), generator=g).float()
             if ints else torch.rand(ids.numel(), generator=g) + 0.5)
    return table, ids, bo, offsets, w


def _bound(table, ids, bo, offsets, w, scale64):
    """(2 len + 4) * 2^-24 * sum |w row| * |scale| per bag and column."""
    flat = R.flat_ids_of(ids, bo, offsets)
    absw = w.double().abs() if w is not None else torch.ones(ids.numel(),
                                                             dtype=torch.float64)
    abssum, _ = R.segment_ref64(table.abs(), flat, bo, absw)
    lens = (bo[1:] - bo[:-1]).double()
    return ((2 * lens + 4) * 2.0 ** -24
            * scale64.abs()).unsqueeze(1) * abssum


@pytest.mark.parametrize("weights", [False, True])
@pytest.mark.parametrize("combiner", R.COMBINERS)
def test_fwd_matches_float64_loop(combiner, weights):
    table, ids, bo, offsets, w = _case(weights=weights)
    if weights:
        w[bo[3]:bo[3] + 2] = torch.tensor([1.0, -1.0])  # zero "mean" sum
    acc, scale = R.loop_ref64(table, ids, bo, NF, offsets, w, combiner)
    out, bag_scale, flat = ops.emb_bag_fwd(table, ids, bo, NF,
                                           offsets=offsets, weights=w,
                                           combiner=combiner)
    assert out.shape == (4, NF * DIM) and out.dtype == torch.float32
    assert torch.equal(flat, R.flat_ids_of(ids, bo, offsets))
    if not (weights and combiner != "sum"):
        R.assert_scale_1ulp(bag_scale, scale)  # exact denominators
    else:
        assert torch.allclose(bag_scale.double(), scale, rtol=1e-5, atol=0)
    want = (acc * scale.unsqueeze(1))
    err = (out.reshape(-1, DIM).double() - want).abs()
    assert bool((err <= _bound(table, ids, bo, offsets, w, scale)).all())
    empty = (bo[1:] == bo[:-1])
    assert empty[0] and empty[4] and empty[-1]
    assert torch.equal(out.reshape(-1, DIM)[empty],
                       torch.zeros(int(empty.sum()), DIM))
    assert torch.equal(bag_scale[empty], torch.zeros(int(empty.sum())))
    if weights and combiner == "mean":
        assert bag_scale[3] == 0 and not out.reshape(-1, DIM)[3].any()


@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("weights", [False, True])
@pytest.mark.parametrize("combiner", R.COMBINERS)
def test_fwd_exact_on_integers(combiner, weights, out_dtype):
    """Integer operands: the sums are exact, so ``out`` is the float64
    sum times the returned scale, rounded once; ``col_offset`` leaves the
    columns on both sides alone."""
    exact_ints.assert_exact(8, 4, max(LENGTHS))
    table, ids, bo, offsets, w = _case(seed=1, ints=True, weights=weights)
    acc, scale = R.loop_ref64(table, ids, bo, NF, offsets, w, combiner)
    col, spare = 8, 5
    out = torch.full((4, col + NF * DIM + spare), -77.0, dtype=out_dtype)
    got, bag_scale, _ = ops.emb_bag_fwd(table, ids, bo, NF, offsets=offsets,
                                        weights=w, combiner=combiner,
                                        out=out, col_offset=col)
    assert got is out
    R.assert_scale_1ulp(bag_scale, scale)
    want = (acc.float() * bag_scale.unsqueeze(1)).reshape(4, NF * DIM)
    assert torch.equal(out[:, col:col + NF * DIM], want.to(out_dtype))
    if combiner == "sum":
        assert torch.equal(out[:, col:col + NF * DIM].double(),
                           exact_ints.rne_bf16(acc).double().reshape(4, -1)
                           if out_dtype == torch.bfloat16
                           else acc.reshape(4, -1))
    assert bool((out[:, :col] == -77).all())
    assert bool((out[:, col + NF * DIM:] == -77).all())


def test_raw_ids_with_offsets_equal_pre_added_ids():
    table, ids, bo, offsets, w = _case(seed=2, weights=True)
    a = ops.emb_bag_fwd(table, ids, bo, NF, offsets=offsets, weights=w,
                        combiner="sqrtn")
    flat = R.flat_ids_of(ids, bo, offsets)
    b = ops.emb_bag_fwd(table, flat, bo, NF, weights=w, combiner="sqrtn")
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.equal(a[2], flat) and b[2] is flat


def test_repeated_id_inside_a_bag_counts_twice():
    table = torch.arange(12.0).reshape(3, 4)
    ids = torch.tensor([2, 2, 1])
    bo = torch.tensor([0, 3])
    out, scale, _ = ops.emb_bag_fwd(table, ids, bo, 1, combiner="mean")
    assert torch.equal(out, ((2 * table[2] + table[1])
                             * scale[0]).reshape(1, 4))
    g = torch.tensor([[3.0, -6.0, 9.0, 12.0]])
    rows = ops.emb_bag_bwd_rows(g, bo, scale, 4, 1)
    assert torch.equal(rows, (g * scale[0]).expand(3, 4))


def test_nnz_zero():
    table = torch.randn(sum(SIZES), DIM)
    ids = torch.zeros(0, dtype=torch.int64)
    bo = torch.zeros(2 * NF + 1, dtype=torch.int64)
    out = torch.full((2, NF * DIM + 2), 5.0)
    _, scale, flat = ops.emb_bag_fwd(table, ids, bo, NF, combiner="mean",
                                     out=out, col_offset=2,
                                     weights=torch.zeros(0))
    assert not out[:, 2:].any() and bool((out[:, :2] == 5).all())
    assert not scale.any() and flat.numel() == 0
    rows = ops.emb_bag_bwd_rows(torch.randn(2, NF * DIM + 2), bo, scale,
                                DIM, NF, col_offset=2)
    assert rows.shape == (0, DIM)


@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16])
def test_one_entry_sum_is_emb_fwd_into(out_dtype):
    g = _gen(3)
    table = torch.randn(sum(SIZES), DIM, generator=g)
    ids, bo, offsets = R.make_bags([1] * (5 * NF), SIZES, g)
    flat = R.flat_ids_of(ids, bo, offsets)
    want = torch.full((5, 16 + NF * DIM), 2.0, dtype=out_dtype)
    ops.emb_fwd_into(table, flat, want, 16)
    out = torch.full((5, 16 + NF * DIM), 2.0, dtype=out_dtype)
    ops.emb_bag_fwd(table, ids, bo, NF, offsets=offsets, out=out,
                    col_offset=16)
    assert torch.equal(out, want)


@pytest.mark.parametrize("combiner,weights", [
    ("sum", False), ("mean", False),
    ("sum", True),  # F.embedding_bag has no weighted mean
])
def test_agrees_with_torch_embedding_bag(combiner, weights):
    g = _gen(4)
    table = torch.randn(9, 8, generator=g)
    lengths = [2, 1, 4, 3, 1, 6]  # torch's mean of an empty bag is 0 too
    ids, bo, _ = R.make_bags(lengths, [9], g)
    w = torch.rand(ids.numel(), generator=g) + 0.5 if weights else None
    out, _, _ = ops.emb_bag_fwd(table, ids, bo, 1, weights=w,
                                combiner=combiner)
    want = F_.embedding_bag(ids, table, bo[:-1], mode=combiner,
                            per_sample_weights=w)
    assert torch.allclose(out, want, rtol=1e-6, atol=1e-7)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("weights", [False, True])
@pytest.mark.parametrize("combiner", R.COMBINERS)
def test_bwd_rows(combiner, weights, dtype):
    table, ids, bo, offsets, w = _case(seed=5, weights=weights)
    _, scale, _ = ops.emb_bag_fwd(table, ids, bo, NF, offsets=offsets,
                                  weights=w, combiner=combiner)
    col = 3
    grad = torch.randn(4, col + NF * DIM + 2, generator=_gen(6)).to(dtype)
    rows = ops.emb_bag_bwd_rows(grad, bo, scale, DIM, NF, weights=w,
                                col_offset=col)
    assert rows.dtype == dtype and rows.shape == (ids.numel(), DIM)
    bag = R.bag_of_entry(bo)
    g = grad[:, col:col + NF * DIM].reshape(-1, DIM)[bag]
    if combiner == "sum" and not weights:
        assert torch.equal(rows, g)
        return
    s = scale[bag] * w if weights else scale[bag]
    assert torch.equal(rows, (g.float() * s.unsqueeze(1)).to(dtype))
    want64 = g.double() * (scale.double()[bag] * (w.double() if weights
                                                  else 1.0)).unsqueeze(1)
    tol = 2.0 ** -7 if dtype == torch.bfloat16 else 2.0 ** -22
    assert bool(((rows.double() - want64).abs()
                 <= tol * want64.abs() + 1e-30).all())


# ---- modules ---------------------------------------------------------------

def _dyadic_bags(seed, batch):
    """Multi-hot batch with power-of-two weights: every product ``w_i *
    row_i`` is exact, so ``fmaf`` and multiply-then-add agree to the bit
    and a torch loop in entry order reproduces the pooled values."""
    g = _gen(seed)
    lengths = torch.randint(0, 5, (batch * NF,), generator=g)
    lengths[1] = 0
    ids, bo, offsets = R.make_bags(lengths, SIZES, g)
    w = 2.0 ** torch.randint(-1, 2, (ids.numel(),), generator=g).float()
    return ids, bo, offsets, w


def _pool_with_torch(table, flat, bo, w, combiner, dim):
    """Pooled bags by a torch loop, and the per-entry scale ``s_i``."""
    n_bags = bo.numel() - 1
    pooled = torch.zeros(n_bags, dim)
    scale = torch.zeros(n_bags)
    for k in range(n_bags):
        lo, hi = int(bo[k]), int(bo[k + 1])
        if hi == lo:
            continue
        acc = torch.zeros(dim)
        for i in range(lo, hi):
            acc = acc + w[i] * table[flat[i]]
        ww = w[lo:hi]
        if combiner == "mean":
            scale[k] = torch.ones(()) / ww.sum()
        elif combiner == "sqrtn":  # the definition: via float64, one rounding
            scale[k] = (1.0 / (ww * ww).sum().double().sqrt()).float()
        else:
            scale[k] = 1.0
        pooled[k] = acc * scale[k] if combiner != "sum" else acc
    return pooled, scale[R.bag_of_entry(bo)] * w


def _apply_rule(rule, lr, table, states, flat, rows, wide, step):
    """The existing update op of ``rule`` on an expanded update list."""
    if rule == "sgd":
        if wide:
            ops.emb_scatter_sum(table, flat.reshape(-1, 1), rows, alpha=-lr)
        else:
            ops.emb_bwd_sgd(table, flat, rows, lr=lr)
        return
    kw = {"lazy_adam": dict(step=step, eps=1e-10)}.get(rule, {})
    if rule == "rowwise_adagrad":
        ops.emb_bwd_rowwise_adagrad(table, *states, flat, rows, lr=lr)
        return
    fn = getattr(ops, f"emb_bwd_{rule}" + ("_wide" if wide else ""))
    fn(table, *states, flat, rows, lr=lr, **kw)


_STATE_NAMES = {
    "sgd": (), "adagrad": ("state_sum",),
    "rowwise_adagrad": ("state_sum_row",),
    "ftrl": ("ftrl_accum", "ftrl_linear"),
    "lazy_adam": ("adam_exp_avg", "adam_exp_avg_sq"),
}


def _states_of(module, rule):
    return [getattr(module, n) for n in _STATE_NAMES[rule]]


@pytest.mark.parametrize("combiner", ["mean", "sqrtn"])
@pytest.mark.parametrize("rule", RULES)
def test_sparse_embedding_two_steps(rule, combiner):
    torch.manual_seed(0)
    emb = SparseEmbedding(SIZES, DIM, sparse_optimizer=rule,
                          combiner=combiner, sparse_initial_accumulator=0.1)
    table = emb.weight.detach().clone()
    states = [s.clone() for s in _states_of(emb, rule)]
    lr = 0.25
    for step in (1, 2):
        ids, bo, offsets, w = _dyadic_bags(10 + step, batch=3)
        up = torch.randn(3, NF * DIM, generator=_gen(20 + step))
        out = emb(ids, bo, w)
        flat = R.flat_ids_of(ids, bo, offsets)
        pooled, s = _pool_with_torch(table, flat, bo, w, combiner, DIM)
        assert torch.equal(out.detach(), pooled.reshape(3, -1))
        (out * up).sum().backward()
        (entry,) = emb.pending_grads()
        assert isinstance(entry, BagUpdate)
        rows = up.reshape(-1, DIM)[R.bag_of_entry(bo)] * s.unsqueeze(1)
        assert torch.equal(entry.flat_ids, flat)
        assert torch.equal(entry.grad_rows, rows)
        emb.apply_sparse_updates(lr)
        assert not emb.pending_grads()
        _apply_rule(rule, lr, table, states, flat, rows, False, step)
        assert torch.equal(emb.weight.detach(), table)
        for got, want in zip(_states_of(emb, rule), states):
            assert torch.equal(got, want)


@pytest.mark.parametrize("rule", RULES)
def test_wide_and_deep_two_steps(rule):
    torch.manual_seed(1)
    wide_rule = "adagrad" if rule == "rowwise_adagrad" else rule
    model = WideAndDeep(table_sizes=SIZES, embedding_dim=DIM, hidden=(8, 4),
                        sparse_optimizer=rule, combiner="mean",
                        sparse_initial_accumulator=0.1)
    hand = copy.deepcopy(model)
    d, wd_ = hand.deep_embedding, hand.wide_embedding
    lr = 0.25
    pad = _DeepInput.DENSE_PAD
    for step in (1, 2):
        ids, bo, offsets, w = _dyadic_bags(30 + step, batch=4)
        g = _gen(40 + step)
        dense = torch.randn(4, 13, generator=g)
        labels = (torch.rand(4, generator=g) < 0.5).float()
        loss = model(dense, ids, labels=labels, bag_offsets=bo,
                     sparse_weights=w)
        loss.backward()
        model.apply_sparse_updates(lr)
        # by hand: pool with torch, run the same tower, expand, update
        flat = R.flat_ids_of(ids, bo, offsets)
        with torch.no_grad():
            pooled, s = _pool_with_torch(d.weight, flat, bo, w, "mean", DIM)
            wpooled, _ = _pool_with_torch(wd_.weight, flat, bo, w, "mean", 1)
        pooled = pooled.reshape(4, -1).requires_grad_()
        wpooled = wpooled.reshape(4, NF).requires_grad_()
        deep_in = torch.cat([dense, torch.zeros(4, pad - 13), pooled], 1)
        hand_loss = ops.bce_head_loss(hand._deep_tower(deep_in),
                                      wpooled.sum(dim=1),
                                      hand.wide_dense(dense), labels)
        assert torch.equal(loss.detach(), hand_loss.detach())
        hand_loss.backward()
        bag = R.bag_of_entry(bo)
        rows = pooled.grad.reshape(-1, DIM)[bag] * s.unsqueeze(1)
        wrows = wpooled.grad.reshape(-1)[bag] * s
        with torch.no_grad():
            _apply_rule(rule, lr, d.weight, _states_of(d, rule), flat, rows,
                        False, step)
            _apply_rule(wide_rule, lr, wd_.weight,
                        _states_of(wd_, wide_rule), flat, wrows, True, step)
        for a, b in ((model.deep_embedding, d), (model.wide_embedding, wd_)):
            r = rule if a is model.deep_embedding else wide_rule
            assert torch.equal(a.weight, b.weight)
            for got, want in zip(_states_of(a, r), _states_of(b, r)):
                assert torch.equal(got, want)
    assert sorted(model.state_dict()) == sorted(hand.state_dict())


def test_wide_and_deep_second_step_uses_updated_tables():
    """Two full steps with exact (integer) arithmetic, where step two's
    forward cannot round differently: tables after both steps equal the
    hand-expanded ones."""
    g = _gen(7)
    model = R.int_model(SIZES, DIM, (4,), g, sparse_optimizer="sgd")
    hand = copy.deepcopy(model)
    d, wd_ = hand.deep_embedding, hand.wide_embedding
    for step in (1, 2):
        lengths = torch.randint(0, 4, (3 * NF,), generator=g)
        ids, bo, offsets = R.make_bags(lengths, SIZES, g)
        dense = torch.randint(-1, 2, (3, 13), generator=g).float()
        model(dense, ids, bag_offsets=bo).sum().backward()
        model.apply_sparse_updates(1.0)
        flat = R.flat_ids_of(ids, bo, offsets)
        bag = R.bag_of_entry(bo)
        with torch.no_grad():
            pooled = torch.zeros(3 * NF, DIM).index_add_(
                0, bag, d.weight[flat])
            wpooled = torch.zeros(3 * NF, 1).index_add_(
                0, bag, wd_.weight[flat])
        pooled = pooled.reshape(3, -1).requires_grad_()
        wpooled = wpooled.reshape(3, NF).requires_grad_()
        deep_in = torch.cat([dense, torch.zeros(3, 3), pooled], 1)
        (hand._deep_tower(deep_in) + wpooled.sum(dim=1)
         + hand.wide_dense(dense)).sum().backward()
        with torch.no_grad():
            ops.emb_bwd_sgd(d.weight, flat,
                            pooled.grad.reshape(-1, DIM)[bag], lr=1.0)
            ops.emb_scatter_sum(wd_.weight, flat.reshape(-1, 1),
                                wpooled.grad.reshape(-1)[bag], alpha=-1.0)
        assert torch.equal(model.deep_embedding.weight, d.weight), step
        assert torch.equal(model.wide_embedding.weight, wd_.weight), step


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_length_one_bags_are_the_one_hot_call(dtype):
    torch.manual_seed(2)
    a = WideAndDeep(table_sizes=SIZES, embedding_dim=DIM, hidden=(8,),
                    compute_dtype=dtype)
    b = copy.deepcopy(a)
    g = _gen(8)
    ids2d = torch.stack([torch.randint(0, s, (6,), generator=g)
                         for s in SIZES], 1)
    dense = torch.randn(6, 13, generator=g)
    labels = (torch.rand(6, generator=g) < 0.5).float()
    la = a(dense, ids2d, labels=labels)
    lb = b(dense, ids2d.reshape(-1), labels=labels,
           bag_offsets=torch.arange(6 * NF + 1))
    assert torch.equal(la, lb)
    la.backward()
    lb.backward()
    a.apply_sparse_updates(0.5)
    b.apply_sparse_updates(0.5)
    for pa, pb in zip(a.state_dict().values(), b.state_dict().values()):
        assert torch.equal(pa, pb)
    for pa, pb in zip(a.parameters(), b.parameters()):
        if pa.grad is not None:
            assert torch.equal(pa.grad, pb.grad)


# ---- host-side refusals ----------------------------------------------------

def test_host_checks_raise():
    table, ids, bo, offsets, _ = _case()
    with pytest.raises(ValueError, match="bag_offsets"):
        ops.emb_bag_fwd(table, ids, bo[:-1], NF, offsets=offsets)
    with pytest.raises(ValueError, match="weights"):
        ops.emb_bag_fwd(table, ids, bo, NF, offsets=offsets,
                        weights=torch.ones(ids.numel() + 1))
    with pytest.raises(ValueError, match="combiner"):
        ops.emb_bag_fwd(table, ids, bo, NF, offsets=offsets,
                        combiner="max")
    with pytest.raises(ValueError, match="does not fit"):
        ops.emb_bag_fwd(table, ids, bo, NF, offsets=offsets,
                        out=torch.zeros(4, NF * DIM + 3), col_offset=4)
    with pytest.raises(ValueError, match="combiner"):
        SparseEmbedding(SIZES, DIM, combiner="max")
    with pytest.raises(ValueError, match="combiner"):
        WideAndDeep(table_sizes=SIZES, embedding_dim=DIM, combiner="avg")
    _, scale, _ = ops.emb_bag_fwd(table, ids, bo, NF, offsets=offsets)
    with pytest.raises(ValueError, match="weights"):
        ops.emb_bag_bwd_rows(torch.zeros(4, NF * DIM), bo, scale, DIM, NF,
                             weights=torch.ones(3), nnz=ids.numel())


def test_sharded_with_bags_is_refused():
    model = WideAndDeep(table_sizes=SIZES, embedding_dim=DIM, hidden=(8,),
                        sharded=True)
    _, ids, bo, _, _ = _case()
    with pytest.raises(NotImplementedError, match="all-to-all"):
        model(torch.zeros(4, 13), ids, bag_offsets=bo)


def test_debug_bounds_refuse_malformed_input(monkeypatch):
    monkeypatch.setenv("MIYARN_DEBUG_BOUNDS", "1")
    table, ids, bo, offsets, _ = _case()
    ops.emb_bag_fwd(table, ids, bo, NF, offsets=offsets)  # well-formed
    bad = bo.clone()
    bad[5], bad[6] = bo[6], bo[5] - 1
    assert bad[6] < bad[5]
    with pytest.raises(RuntimeError, match="non-decreasing"):
        ops.emb_bag_fwd(table, ids, bad, NF, offsets=offsets)
    short = bo.clone()
    short[-1] -= 1
    with pytest.raises(RuntimeError, match="end at nnz"):
        ops.emb_bag_fwd(table, ids, short, NF, offsets=offsets)
    big = ids.clone()
    big[-1] = sum(SIZES)  # past the last table row whatever the feature
    with pytest.raises(RuntimeError, match="out of range"):
        ops.emb_bag_fwd(table, big, bo, NF, offsets=offsets)


# ---- two gloo ranks with different nnz -------------------------------------

DP_B = 3
DP_LENGTHS = ([2, 0, 1, 3, 1, 0, 1, 2, 4],     # rank 0: nnz 14
              [1, 1, 0, 0, 2, 1, 0, 1, 0])     # rank 1: nnz 6
DP_LR = 0.5


def _dp_model(rule):
    """Integer parameters (``exact_ints``' regime: every sum below 2**24
    is exact in any order), so the gathered order cannot matter."""
    exact_ints.assert_exact(2, 4, sum(map(sum, DP_LENGTHS)))
    return R.int_model(SIZES, DIM, (4,), _gen(50), sparse_optimizer=rule,
                       sparse_initial_accumulator=0.1, sparse_l1=0.0)


def _dp_batch(rank):
    g = _gen(60 + rank)
    # raw ids >= 1: flat row 0 is touched by nobody, so padding that
    # reached an update op would show there (FTRL recomputes a touched
    # row from its state even under a zero gradient)
    ids, bo, _ = R.make_bags(DP_LENGTHS[rank], SIZES, g, id_lo=1)
    dense = torch.randint(-1, 2, (DP_B, 13), generator=g).float()
    return dense, ids, bo


def _dp_tables(model):
    out = {}
    for name, t in model.state_dict().items():
        if "embedding" in name:
            out[name] = t.detach().clone()
    return out


def _dp_worker(rank, world, kv_addr, rule, out_q):
    from tf_yarn_amd.kv import KVClient
    from tf_yarn_amd.parallel import comm
    comm.init_process_group(rank=rank, world_size=world, backend="gloo",
                            kv_client=KVClient(kv_addr))
    try:
        model = _dp_model(rule)
        dense, ids, bo = _dp_batch(rank)
        model(dense, ids, bag_offsets=bo).sum().backward()
        model.apply_sparse_updates(DP_LR)
        out_q.put((rank, {k: v.tolist()
                          for k, v in _dp_tables(model).items()}))
    finally:
        comm.destroy_process_group()


@pytest.mark.parametrize("rule", ["sgd", "ftrl"])
@pytest.mark.timeout(240)
def test_two_ranks_with_different_nnz_match_one_process(rule):
    from tf_yarn_amd.kv import KVServer
    # one process, the concatenated batch; each rank's loss is its own sum
    # and the gathered update is scaled by 1/world, hence the 0.5
    model = _dp_model(rule)
    parts = [_dp_batch(r) for r in range(2)]
    nnz0 = parts[0][1].numel()
    assert nnz0 != parts[1][1].numel()
    dense = torch.cat([p[0] for p in parts])
    ids = torch.cat([p[1] for p in parts])
    bo = torch.cat([parts[0][2], parts[1][2][1:] + nnz0])
    before = _dp_tables(model)
    (model(dense, ids, bag_offsets=bo).sum() * 0.5).backward()
    model.apply_sparse_updates(DP_LR)
    want = _dp_tables(model)
    assert not torch.equal(want["deep_embedding.weight"],
                           before["deep_embedding.weight"])
    assert torch.equal(want["deep_embedding.weight"][0],
                       before["deep_embedding.weight"][0])

    server = KVServer()
    ctx = mp.get_context("spawn")
    out_q = ctx.Queue()
    procs = [ctx.Process(target=_dp_worker,
                         args=(r, 2, server.address, rule, out_q))
             for r in range(2)]
    for p in procs:
        p.start()
    results = {}
    try:
        for _ in range(2):
            rank, tables = out_q.get(timeout=180)
            results[rank] = tables
    finally:
        for p in procs:
            p.join(timeout=30)
            if p.is_alive():
                p.terminate()
        server.stop()
    for rank in range(2):
        assert sorted(results[rank]) == sorted(want)
        for name, t in want.items():
            got = torch.tensor(results[rank][name], dtype=t.dtype)
            assert torch.equal(got.reshape(t.shape), t), (rank, name)
