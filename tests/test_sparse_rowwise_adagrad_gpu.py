"""Row-wise sparse Adagrad HIP kernels vs the CPU reference op.

Gradients are ``randint(-hi, hi + 1) / 8`` and the scale is 0.5 or 1:
exact in bf16 and fp32, every partial sum a small multiple of
``scale / 8``, so the summed gradient ``G`` is the same in ANY summation
order (``tests/test_sparse_adagrad_gpu.py``).  Here ``G^2`` is also a
multiple of ``(scale / 8)^2``, and the row's sum of squares is exact in
fp32 in any lane order while ``sum_c G^2 / (scale / 8)^2 < 2^24``;
``_exact_case`` computes that quantity in float64 and asserts it for every
case.  What is left between GPU and CPU is sqrt/div rounding and FMA
contraction, the class the element-wise sparse Adagrad tests hold to
``torch.allclose(atol=1e-5)`` against the CPU op; the same call is used
for table and state here."""

import collections

import pytest
import torch

from tf_yarn_amd import ops
from tf_yarn_amd.models.synthetic import synthetic_criteo_batch
from tf_yarn_amd.models.wide_deep import WideAndDeep

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X"),
]

LR, WIDE_LR = 0.05, 0.5
L1, L2 = 0.5, 0.25
Z_MARGIN = 1e-4
DTYPES = [torch.float32, torch.bfloat16]


def _close(gpu, cpu):
    return torch.allclose(gpu.cpu(), cpu, atol=1e-5)


def _exact_grads(gen, shape, dtype, hi=32):
    g = torch.randint(-hi, hi + 1, shape, generator=gen).float() / 8
    return g.to(dtype)


def _assert_row_sums_exact(ids, grad):
    """max over the unique ids of sum_c G^2 / (scale/8)^2, in float64: the
    integer the fp32 sum of squares has to hold, so it must be < 2^24."""
    flat = ids.reshape(-1)
    uniq, inv = torch.unique(flat, return_inverse=True)
    ints = torch.zeros(uniq.numel(), grad.shape[-1], dtype=torch.float64)
    ints.index_add_(0, inv, grad.reshape(flat.numel(), -1).double() * 8)
    worst = float((ints * ints).sum(dim=1).max())
    assert worst < 2 ** 24, worst
    return worst


def _exact_case(rows, dim, n, dtype, seed, id_hi=None, hi=32):
    gen = torch.Generator().manual_seed(seed)
    table = torch.randn(rows, dim, generator=gen)
    state = torch.rand(rows, generator=gen)
    ids = torch.randint(0, id_hi or rows, (n,), generator=gen)
    grad = _exact_grads(gen, (n, dim), dtype, hi)
    _assert_row_sums_exact(ids, grad)
    return table, state, ids, grad


def _run_both(table, state, ids, grad, scale=1.0, workspace=None):
    """Apply on a GPU copy (returned) and in place on the CPU tensors."""
    tg, sg = table.cuda(), state.cuda()
    ws = workspace or ops.SparseWorkspace(tg)
    ops.emb_bwd_rowwise_adagrad(tg, sg, ids.cuda(), grad.cuda(), lr=LR,
                                scale=scale, workspace=ws)
    ops.emb_bwd_rowwise_adagrad(table, state, ids, grad, lr=LR, scale=scale)
    return tg, sg, ws


# dims 4..256: the lane-sharing kernel, dvec 1 (no shuffle partner, 16 rows
# per wave) to 64 (one row is a whole wave, the full butterfly); 1, 7, 12
# and 512 (past dvec = 64): the one-lane-per-row kernel.  n = 1001 leaves a
# tail wave.
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [1000, 1001])
@pytest.mark.parametrize("dim", [4, 16, 64, 256, 1, 7, 12, 512])
def test_apply_matches_reference(dim, n, dtype):
    table, state, ids, grad = _exact_case(500, dim, n, dtype,
                                          seed=dim * 7 + n)
    t0, s0 = table.clone(), state.clone()
    tg, sg, ws = _run_both(table, state, ids, grad, scale=0.5)
    assert sg.shape == (500,)
    assert _close(tg, table) and _close(sg, state)
    assert not ws.acc.any()
    named = torch.zeros(500, dtype=torch.bool)
    named[ids] = True
    assert torch.equal(tg.cpu()[~named], t0[~named])
    assert torch.equal(sg.cpu()[~named], s0[~named])
    assert not torch.equal(sg.cpu()[named], s0[named])


@pytest.mark.parametrize("dtype", DTYPES)
def test_grid_stride_loop_iterates(dtype):
    # n * dim/4 = 2.4M quads > 8192 blocks * 256 threads
    table, state, ids, grad = _exact_case(100_000, 16, 600_000, dtype,
                                          seed=3)
    tg, sg, ws = _run_both(table, state, ids, grad)
    assert _close(tg, table) and _close(sg, state)
    assert not ws.acc.any()


# hi = 8: with randint(-32, 33) the dim-16 case holds 1.1e7 of the 1.7e7
# that fp32 takes exactly, too close to keep
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dim,n", [(16, 4096), (256, 512)])
def test_heavy_collisions(dim, n, dtype):
    table, state, ids, grad = _exact_case(8, dim, n, dtype, seed=1,
                                          id_hi=3, hi=8)
    t0, s0 = table.clone(), state.clone()
    tg, sg, ws = _run_both(table, state, ids, grad)
    assert _close(tg, table) and _close(sg, state)
    assert not ws.acc.any()
    assert torch.equal(tg.cpu()[3:], t0[3:])
    assert torch.equal(sg.cpu()[3:], s0[3:])


@pytest.mark.parametrize("dtype", DTYPES)
def test_many_rows_per_wave(dtype):
    table, state, ids, grad = _exact_case(64, 4, 4096, dtype, seed=2)
    tg, sg, _ = _run_both(table, state, ids, grad)
    assert _close(tg, table) and _close(sg, state)


def _code(ids):
    return (ids * 7) % 11 + 1  # 1..11, differs between neighbouring ids


# Every element of an update row is the small integer code(id), the state
# starts at 0: the row's mean of squares is copies^2 * code^2 EXACTLY, so a
# butterfly that leaks into a neighbouring row, drops a lane or counts a
# loser turns an integer wrong.  copies = 2 names every id twice, so half
# of the update rows are losers that sit among the winners.
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("copies", [1, 2])
@pytest.mark.parametrize("dim", [4, 16])
def test_position_coded_state_is_exact(dim, copies, dtype):
    gen = torch.Generator().manual_seed(dim + copies)
    rows = 64
    ids = torch.cat([torch.randperm(rows, generator=gen)
                     for _ in range(copies)])
    grad = _code(ids).float().reshape(-1, 1).expand(-1, dim).contiguous()
    grad = grad.to(dtype)
    table = torch.randn(rows, dim, generator=gen)
    state = torch.zeros(rows)
    tg, sg, ws = _run_both(table, state, ids, grad)
    want = (copies * _code(torch.arange(rows))).float() ** 2
    assert torch.equal(sg.cpu(), want)
    assert torch.equal(state, want)
    assert _close(tg, table)
    assert not ws.acc.any()


@pytest.mark.parametrize("dim", [16, 256, 1, 12])
def test_workspace_cleans_itself_over_three_steps(dim):
    gen = torch.Generator().manual_seed(4)
    table = torch.randn(400, dim, generator=gen)
    state = torch.zeros(400)
    t0, s0 = table.clone(), state.clone()
    tg, sg = table.cuda(), state.cuda()
    ws = ops.SparseWorkspace(tg)
    for step in range(3):
        # overlapping ids, even rows only
        ids = torch.randint(0, 100, (777,), generator=gen) * 2
        grad = _exact_grads(gen, (777, dim), torch.float32)
        _assert_row_sums_exact(ids, grad)
        ops.emb_bwd_rowwise_adagrad(tg, sg, ids.cuda(), grad.cuda(), lr=LR,
                                    workspace=ws)
        ops.emb_bwd_rowwise_adagrad(table, state, ids, grad, lr=LR)
        assert not ws.acc.any(), f"accumulator dirty after step {step}"
        assert ws.epoch == step + 1
        assert _close(tg, table) and _close(sg, state), step
    untouched = torch.cat([torch.arange(1, 400, 2),
                           torch.arange(200, 400)])
    assert torch.equal(tg.cpu()[untouched], t0[untouched])
    assert torch.equal(sg.cpu()[untouched], s0[untouched])


def _zeros_agree(w_gpu, w_cpu, z_cpu, ids, l1):
    """Same exact-zero set on the touched rows, away from the FTRL
    threshold (``tests/test_sparse_ftrl_gpu.py``)."""
    rows = torch.unique(ids.reshape(-1))
    sure = ((z_cpu[rows].abs() - l1).abs() >= Z_MARGIN)
    assert float((~sure).double().mean()) <= 0.01
    got, want = (w_gpu.cpu()[rows] == 0.0), (w_cpu[rows] == 0.0)
    return torch.equal(got[sure], want[sure])


# dim 12 and mixed grad dtypes take the two single-table kernels
@pytest.mark.parametrize("dim,mixed", [(16, False), (64, False),
                                       (12, False), (16, True)])
@pytest.mark.parametrize("g_div", [4, 26])
@pytest.mark.parametrize("wide_rule", ["adagrad", "ftrl"])
def test_fused_deep_wide(wide_rule, g_div, dim, mixed):
    gen = torch.Generator().manual_seed(6 + g_div)
    rows, b = 500, 41
    n = b * g_div
    deep = (torch.randn(rows, dim, generator=gen),
            torch.rand(rows, generator=gen))
    wide = (torch.randn(rows, 1, generator=gen),
            torch.rand(rows, 1, generator=gen) + 0.1)
    if wide_rule == "ftrl":
        wide += (torch.randn(rows, 1, generator=gen) * 0.1,)
    ids = torch.randint(0, rows, (n,), generator=gen)
    grad = _exact_grads(gen, (n, dim), torch.bfloat16)
    _assert_row_sums_exact(ids, grad)
    gw = _exact_grads(gen, (b,),
                      torch.float32 if mixed else torch.bfloat16)
    dev = [t.cuda() for t in deep + wide]
    ws = ops.SparseWorkspace(dev[0], dev[2])
    for _ in range(2):  # second call: stamps of the first must not block
        if wide_rule == "adagrad":
            ops.emb_bwd_rowwise_adagrad_fused_wide(
                *dev, ids.cuda(), grad.cuda(), gw.cuda(), lr=LR, scale=0.5,
                workspace=ws)
            ops.emb_bwd_adagrad_wide(*wide, ids, gw, lr=LR, scale=0.5)
        else:
            ops.emb_bwd_rowwise_adagrad_ftrl_fused_wide(
                *dev, ids.cuda(), grad.cuda(), gw.cuda(), lr=LR,
                wide_lr=WIDE_LR, l1=L1, l2=L2, scale=0.5, workspace=ws)
            ops.emb_bwd_ftrl_wide(*wide, ids, gw, lr=WIDE_LR, l1=L1, l2=L2,
                                  scale=0.5)
        ops.emb_bwd_rowwise_adagrad(*deep, ids, grad, lr=LR, scale=0.5)
    for got, want in zip(dev, deep + wide):
        assert _close(got, want)
    if wide_rule == "ftrl":
        assert _zeros_agree(dev[2], wide[0], wide[2], ids, L1)
    assert not ws.acc.any() and not ws.wide_acc.any()
    assert ws.epoch == (2 if dim != 12 and not mixed else 4)


# pass 2 has no float atomics and the inputs make pass 1 exact
@pytest.mark.parametrize("dim", [16, 12])
def test_two_gpu_runs_agree_bit_for_bit(dim):
    table, state, ids, grad = _exact_case(500, dim, 3000, torch.bfloat16,
                                          seed=8)
    runs = []
    for _ in range(2):
        tg, sg = table.cuda(), state.cuda()
        ops.emb_bwd_rowwise_adagrad(tg, sg, ids.cuda(), grad.cuda(), lr=LR,
                                    scale=0.5)
        runs.append((tg.cpu(), sg.cpu()))
    assert torch.equal(runs[0][0], runs[1][0])
    assert torch.equal(runs[0][1], runs[1][1])
    assert not torch.equal(runs[0][0], table)


class _Counted:
    """``_C.emb_bwd_sparse``, counting calls by (deep rule, wide rule)."""

    def __init__(self, fn):
        self.fn, self.calls = fn, collections.Counter()

    def __call__(self, deep, wide, *args):
        self.calls[(deep and deep[0], wide and wide[0])] += 1
        return self.fn(deep, wide, *args)


@pytest.mark.parametrize("wide_rule", ["adagrad", "ftrl"])
@pytest.mark.parametrize("sharded", [False, True])
def test_model_update_runs_the_hip_kernels(sharded, wide_rule, monkeypatch):
    torch.manual_seed(7)
    tables = [50] * 4
    l1, l2 = 0.001, 0.01
    ftrl = wide_rule == "ftrl"
    model = WideAndDeep(table_sizes=tables, embedding_dim=16,
                        hidden=(64, 32), compute_dtype=torch.bfloat16,
                        sharded=sharded, sparse_optimizer="rowwise_adagrad",
                        wide_sparse_optimizer="ftrl" if ftrl else None,
                        sparse_l1=l1, sparse_l2=l2,
                        wide_sparse_lr=WIDE_LR if ftrl else None,
                        sparse_initial_accumulator=0.1).cuda()
    assert model.wide_sparse_optimizer == wide_rule
    counted = _Counted(ops._C.emb_bwd_sparse)
    monkeypatch.setattr(ops._C, "emb_bwd_sparse", counted)
    wide_names = ["ftrl_accum", "ftrl_linear"] if ftrl else ["state_sum"]
    if sharded:
        e = model.embeddings
        params = [e.weight, e.state_sum_row, e.wide_weight] + \
            [getattr(e, "wide_" + n) for n in wide_names]
        sinks = (e._deep_sink, e._wide_sink)
        assert not hasattr(e, "state_sum")
    else:
        d, w = model.deep_embedding, model.wide_embedding
        params = [d.weight, d.state_sum_row, w.weight] + \
            [getattr(w, n) for n in wide_names]
        sinks = (d.pending_grads(), w.pending_grads())
        assert not hasattr(d, "state_sum")
    assert params[1].shape == (sum(tables),)
    for step in range(2):
        dense, ids, labels = synthetic_criteo_batch(
            256, tables, device="cuda", seed=step)
        model(dense, ids % 12, labels=labels).backward()
        (d_ids, d_grad), = [(i.cpu(), g.float().cpu()) for i, g in sinks[0]]
        (w_ids, w_grad), = [(i.cpu(), g.float().cpu()) for i, g in sinks[1]]
        want = [p.detach().cpu().clone() for p in params]
        model.apply_sparse_updates(LR)
        ops.emb_bwd_rowwise_adagrad(
            want[0], want[1], d_ids, d_grad.reshape(d_ids.numel(), -1),
            lr=LR)
        if ftrl:
            ops.emb_bwd_ftrl_wide(*want[2:], w_ids, w_grad, lr=WIDE_LR,
                                  l1=l1, l2=l2)
        else:
            ops.emb_bwd_adagrad_wide(*want[2:], w_ids, w_grad, lr=LR)
        for got, ref in zip(params, want):
            assert _close(got.detach(), ref), step
    if sharded:  # the fused pair alone: no single-table call
        assert counted.calls == {("rowwise_adagrad", wide_rule): 2}
    else:  # the two singles alone: no pair, no element-wise deep Adagrad
        assert counted.calls == {("rowwise_adagrad", None): 2,
                                 (None, wide_rule): 2}
    big = [(name, buf) for name, buf in model.named_buffers()
           if "state_sum" in name or "ftrl" in name or "_adagrad" in name]
    assert len(big) >= 5
    for name, buf in big:
        assert buf.is_cuda and getattr(buf, "_miyarn_sharded", False), name


def _side(table, state_row, acc, grad):
    """A row-wise Adagrad side as ``_C.emb_bwd_sparse`` takes it
    (``grad=None``: pass 2 alone)."""
    return ("rowwise_adagrad", table, [state_row], acc, grad, LR, 1e-10,
            0.0, 0.0)


def test_bad_inputs_raise_before_any_launch():
    table = torch.randn(50, 16).cuda()
    state = torch.zeros(50).cuda()
    ids = torch.randint(0, 50, (40,)).cuda()
    grad = torch.ones(40, 16).cuda()
    ws = ops.SparseWorkspace(table)
    t0 = table.clone()

    def call(table=table, state=state, acc=ws.acc, stamp=ws.stamp, ids=ids,
             grad=grad):
        ops._C.emb_bwd_sparse(_side(table, state, acc, grad), None, stamp,
                              ids, 1, 1.0)

    def apply(**kw):  # pass 2 alone takes the same checks
        kw = dict(dict(table=table, state=state, acc=ws.acc,
                       stamp=ws.stamp, ids=ids), **kw)
        ops._C.emb_bwd_sparse(
            _side(kw["table"], kw["state"], kw["acc"], None), None,
            kw["stamp"], kw["ids"], 1, 1.0)

    bad_state = [
        dict(state=torch.zeros(50, 16).cuda()),       # the table's shape
        dict(state=state.double()),                   # dtype
        dict(state=torch.zeros(100).cuda()[::2]),     # non-contiguous
        dict(state=state[:49].contiguous()),
        dict(state=state.cpu()),
    ]
    bad = bad_state + [
        dict(grad=grad.half()),                       # dtype
        dict(grad=grad.t().contiguous().t()),         # non-contiguous
        dict(grad=grad[:39].contiguous()),            # shape
        dict(table=table.t().contiguous().t()),
        dict(acc=ws.acc[:, :8].contiguous()),
        dict(stamp=ws.stamp.long()),
        dict(stamp=ws.stamp[:49].contiguous()),       # short stamp
        dict(ids=ids.int()),
        dict(ids=torch.arange(80).cuda()[::2]),
    ]
    for kw in bad:
        with pytest.raises(RuntimeError):
            call(**kw)
        if "grad" not in kw:
            with pytest.raises(RuntimeError):
                apply(**kw)
    wide = torch.zeros(50, 1).cuda()
    wws = ops.SparseWorkspace(table, wide)
    gw = torch.ones(10).cuda()

    def pair(state=state, gw=gw, wide_state=torch.zeros_like(wide)):
        ops._C.emb_bwd_sparse(
            _side(table, state, wws.acc, grad),
            ("adagrad", wide, [wide_state], wws.wide_acc, gw, LR, 1e-10,
             0.0, 0.0),
            wws.stamp, ids, 1, 1.0)

    def pair_ftrl(state=state, gw=gw, lr=WIDE_LR):
        ops._C.emb_bwd_sparse(
            _side(table, state, wws.acc, grad),
            ("ftrl", wide, [torch.zeros_like(wide), torch.zeros_like(wide)],
             wws.wide_acc, gw, lr, 1e-10, 0.0, 0.0),
            wws.stamp, ids, 1, 1.0)

    for fn in (pair, pair_ftrl):
        for kw in bad_state:
            with pytest.raises(RuntimeError):
                fn(**kw)
        with pytest.raises(RuntimeError):  # gw dtype differs from grad's
            fn(gw=gw.to(torch.bfloat16))
        with pytest.raises(RuntimeError):  # 40 ids, 7 examples
            fn(gw=torch.ones(7).cuda())
    with pytest.raises(RuntimeError):
        pair(wide_state=torch.zeros(50, 16).cuda())
    with pytest.raises(RuntimeError):
        pair_ftrl(lr=0.0)
    with pytest.raises(RuntimeError):  # the pair kernel does not take dim 12
        t12 = torch.zeros(50, 12).cuda()
        w12 = ops.SparseWorkspace(t12, wide)
        ops._C.emb_bwd_sparse(
            _side(t12, state, w12.acc, torch.ones(40, 12).cuda()),
            ("adagrad", wide, [torch.zeros_like(wide)], w12.wide_acc, gw,
             LR, 1e-10, 0.0, 0.0),
            w12.stamp, ids, 1, 1.0)
    torch.cuda.synchronize()
    assert torch.equal(table, t0)
    assert not state.any() and not ws.acc.any() and not ws.stamp.any()
    assert not wws.acc.any() and not wws.wide_acc.any()
    assert not wws.stamp.any() and not wide.any()
