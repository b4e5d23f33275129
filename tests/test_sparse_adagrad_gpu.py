"""Sparse Adagrad HIP kernels vs the CPU reference op.

Gradients are ``randint(-32, 33) / 8``: exact in bf16 and fp32, and every
partial sum is a multiple of 1/16 far below 2^24/16, so ANY summation
order gives the same fp32 sum — atomic arrival order cannot move the
result.  What is left between GPU and CPU is FMA contraction and
sqrt/div rounding, the class of difference the dense Adagrad kernel test
(``test_fused_adagrad_adadelta_gpu_vs_torch``) covers with
``torch.allclose(..., atol=1e-5)``; the same call is used here."""

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

LR = 0.05


def _close(gpu, cpu):
    return torch.allclose(gpu.cpu(), cpu, atol=1e-5)


def _exact_grads(gen, shape, dtype):
    g = torch.randint(-32, 33, shape, generator=gen).float() / 8
    return g.to(dtype)


def _case(rows, dim, n, dtype, seed, id_hi=None):
    gen = torch.Generator().manual_seed(seed)
    table = torch.randn(rows, dim, generator=gen)
    state = torch.rand(rows, dim, generator=gen)
    ids = torch.randint(0, id_hi or rows, (n,), generator=gen)
    grad = _exact_grads(gen, (n, dim), dtype)
    return table, state, ids, grad


def _run_both(table, state, ids, grad, scale=1.0, workspace=None):
    """Apply on a GPU copy (returned) and in place on the CPU tensors."""
    tg, sg = table.cuda(), state.cuda()
    ws = workspace or ops.SparseAdagradWorkspace(tg)
    ops.emb_bwd_adagrad(tg, sg, ids.cuda(), grad.cuda(), lr=LR,
                        scale=scale, workspace=ws)
    ops.emb_bwd_adagrad(table, state, ids, grad, lr=LR, scale=scale)
    return tg, sg, ws


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("n", [1000, 1001])
@pytest.mark.parametrize("dim", [16, 4, 64, 1, 7, 12])
def test_apply_matches_reference(dim, n, dtype):
    table, state, ids, grad = _case(500, dim, n, dtype, seed=dim * 7 + n)
    tg, sg, ws = _run_both(table, state, ids, grad, scale=0.5)
    assert _close(tg, table) and _close(sg, state)
    assert not ws.acc.any()


def test_heavy_collisions():
    table, state, ids, grad = _case(8, 16, 4096, torch.float32, seed=1,
                                    id_hi=3)
    tg, sg, _ = _run_both(table, state, ids, grad)
    assert _close(tg, table) and _close(sg, state)


def test_many_rows_per_wave():
    table, state, ids, grad = _case(64, 4, 4096, torch.bfloat16, seed=2)
    tg, sg, _ = _run_both(table, state, ids, grad)
    assert _close(tg, table) and _close(sg, state)


def test_grid_stride_loop_iterates():
    # n * dim/4 = 2.4M quads > 8192 blocks * 256 threads
    table, state, ids, grad = _case(100_000, 16, 600_000, torch.bfloat16,
                                    seed=3)
    tg, sg, ws = _run_both(table, state, ids, grad)
    assert _close(tg, table) and _close(sg, state)
    assert not ws.acc.any()


@pytest.mark.parametrize("dim", [16, 1, 12])
def test_workspace_cleans_itself_over_three_steps(dim):
    gen = torch.Generator().manual_seed(4)
    table = torch.randn(400, dim, generator=gen)
    state = torch.zeros(400, dim)
    t0, s0 = table.clone(), state.clone()
    tg, sg = table.cuda(), state.cuda()
    ws = ops.SparseAdagradWorkspace(tg)
    for step in range(3):
        # overlapping ids, even rows only
        ids = torch.randint(0, 100, (777,), generator=gen) * 2
        grad = _exact_grads(gen, (777, dim), torch.float32)
        ops.emb_bwd_adagrad(tg, sg, ids.cuda(), grad.cuda(), lr=LR,
                            workspace=ws)
        ops.emb_bwd_adagrad(table, state, ids, grad, lr=LR)
        assert not ws.acc.any(), f"accumulator dirty after step {step}"
        assert ws.epoch == step + 1
        assert _close(tg, table) and _close(sg, state), step
    untouched = torch.cat([torch.arange(1, 400, 2),
                           torch.arange(200, 400)])
    assert torch.equal(tg.cpu()[untouched], t0[untouched])
    assert torch.equal(sg.cpu()[untouched], s0[untouched])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_wide_companion(dtype):
    gen = torch.Generator().manual_seed(5)
    f, b = 26, 77
    table = torch.randn(500, 1, generator=gen)
    state = torch.rand(500, 1, generator=gen)
    ids = torch.randint(0, 500, (b, f), generator=gen)
    gw = _exact_grads(gen, (b,), dtype)
    tg, sg = table.cuda(), state.cuda()
    ws = ops.SparseAdagradWorkspace(tg)
    ops.emb_bwd_adagrad_wide(tg, sg, ids.cuda(), gw.cuda(), lr=LR,
                             scale=0.5, workspace=ws)
    ops.emb_bwd_adagrad_wide(table, state, ids, gw, lr=LR, scale=0.5)
    assert _close(tg, table) and _close(sg, state)
    assert not ws.acc.any()


# dim 12 and mixed grad dtypes take the two single-table kernels
@pytest.mark.parametrize("dim,mixed", [(16, False), (64, False),
                                       (12, False), (16, True)])
@pytest.mark.parametrize("g_div", [4, 26])
def test_fused_deep_wide(g_div, dim, mixed):
    gen = torch.Generator().manual_seed(6 + g_div)
    rows, b = 500, 41
    n = b * g_div
    deep = torch.randn(rows, dim, generator=gen)
    deep_s = torch.rand(rows, dim, generator=gen)
    wide = torch.randn(rows, 1, generator=gen)
    wide_s = torch.rand(rows, 1, generator=gen)
    ids = torch.randint(0, rows, (n,), generator=gen)
    grad = _exact_grads(gen, (n, dim), torch.bfloat16)
    gw = _exact_grads(gen, (b,),
                      torch.float32 if mixed else torch.bfloat16)
    dev = [t.cuda() for t in (deep, deep_s, wide, wide_s)]
    ws = ops.SparseAdagradWorkspace(dev[0], dev[2])
    for _ in range(2):  # second call: stamps of the first must not block
        ops.emb_bwd_adagrad_fused_wide(*dev, ids.cuda(), grad.cuda(),
                                       gw.cuda(), lr=LR, scale=0.5,
                                       workspace=ws)
        ops.emb_bwd_adagrad(deep, deep_s, ids, grad, lr=LR, scale=0.5)
        ops.emb_bwd_adagrad_wide(wide, wide_s, ids, gw, lr=LR, scale=0.5)
    for got, want in zip(dev, (deep, deep_s, wide, wide_s)):
        assert _close(got, want)
    assert not ws.acc.any() and not ws.wide_acc.any()


class _Counted:
    """``_C.emb_bwd_sparse``, counting calls by (deep rule, wide rule)."""

    def __init__(self, fn):
        self.fn, self.calls = fn, collections.Counter()

    def __call__(self, deep, wide, *args):
        self.calls[(deep and deep[0], wide and wide[0])] += 1
        return self.fn(deep, wide, *args)


@pytest.mark.parametrize("sharded", [False, True])
def test_model_update_runs_the_hip_kernels(sharded, monkeypatch):
    torch.manual_seed(7)
    tables = [50] * 4
    model = WideAndDeep(table_sizes=tables, embedding_dim=16,
                        hidden=(64, 32), compute_dtype=torch.bfloat16,
                        sharded=sharded,
                        sparse_optimizer="adagrad").cuda()
    counted = _Counted(ops._C.emb_bwd_sparse)
    monkeypatch.setattr(ops._C, "emb_bwd_sparse", counted)
    if sharded:
        e = model.embeddings
        params = (e.weight, e.state_sum, e.wide_weight, e.wide_state_sum)
        sinks = (e._deep_sink, e._wide_sink)
    else:
        d, w = model.deep_embedding, model.wide_embedding
        params = (d.weight, d.state_sum, w.weight, w.state_sum)
        sinks = (d.pending_grads(), w.pending_grads())
    for step in range(2):
        dense, ids, labels = synthetic_criteo_batch(
            256, tables, device="cuda", seed=step)
        model(dense, ids % 12, labels=labels).backward()
        (d_ids, d_grad), = [(i.cpu(), g.float().cpu()) for i, g in sinks[0]]
        (w_ids, w_grad), = [(i.cpu(), g.float().cpu()) for i, g in sinks[1]]
        dt, ds, wt, wst = [p.detach().cpu().clone() for p in params]
        model.apply_sparse_updates(LR)
        ops.emb_bwd_adagrad(dt, ds, d_ids,
                            d_grad.reshape(d_ids.numel(), -1), lr=LR)
        ops.emb_bwd_adagrad_wide(wt, wst, w_ids, w_grad, lr=LR)
        for got, want in zip(params, (dt, ds, wt, wst)):
            assert _close(got.detach(), want), step
    if sharded:
        assert counted.calls == {("adagrad", "adagrad"): 2}
    else:
        assert counted.calls == {("adagrad", None): 2, (None, "adagrad"): 2}
    for name, buf in model.named_buffers():
        if "state_sum" in name or "_adagrad" in name:
            assert buf.is_cuda and getattr(buf, "_miyarn_sharded", False)


def _side(table, state, acc, grad):
    """An Adagrad side as ``_C.emb_bwd_sparse`` takes it."""
    return ("adagrad", table, [state], acc, grad, LR, 1e-10, 0.0, 0.0)


def test_bad_inputs_raise_before_any_launch():
    table = torch.randn(50, 16).cuda()
    state = torch.zeros(50, 16).cuda()
    ids = torch.randint(0, 50, (40,)).cuda()
    grad = torch.ones(40, 16).cuda()
    ws = ops.SparseAdagradWorkspace(table)
    t0 = table.clone()

    def call(table=table, state=state, acc=ws.acc, stamp=ws.stamp, ids=ids,
             grad=grad):
        ops._C.emb_bwd_sparse(_side(table, state, acc, grad), None, stamp,
                              ids, 1, 1.0)

    bad = [
        dict(grad=grad.half()),                       # dtype
        dict(grad=grad.t().contiguous().t()),         # non-contiguous
        dict(grad=grad[:39].contiguous()),            # shape
        dict(state=state.double()),
        dict(state=torch.zeros(16, 50).cuda().t()),
        dict(state=state[:49].contiguous()),
        dict(table=table.t().contiguous().t()),
        dict(acc=ws.acc[:, :8].contiguous()),
        dict(stamp=ws.stamp.long()),
        dict(stamp=ws.stamp[:49].contiguous()),
        dict(ids=ids.int()),
        dict(ids=torch.arange(80).cuda()[::2]),
    ]
    for kw in bad:
        with pytest.raises(RuntimeError):
            call(**kw)
    wide = torch.zeros(50, 1).cuda()
    wws = ops.SparseAdagradWorkspace(table, wide)
    with pytest.raises(RuntimeError):  # gw dtype differs from grad's
        ops._C.emb_bwd_sparse(
            _side(table, state, wws.acc, grad),
            _side(wide, torch.zeros_like(wide), wws.wide_acc,
                  torch.ones(10, dtype=torch.bfloat16).cuda()),
            wws.stamp, ids, 1, 1.0)
    with pytest.raises(RuntimeError):  # 40 ids, 7 examples
        ops._C.emb_bwd_sparse(
            None, _side(wide, torch.zeros_like(wide), wws.wide_acc,
                        torch.ones(7).cuda()),
            wws.stamp, ids, 1, 1.0)
    torch.cuda.synchronize()
    assert torch.equal(table, t0)
    assert not state.any() and not ws.acc.any() and not ws.stamp.any()
    assert not wws.acc.any() and not wws.wide_acc.any()
    assert not wws.stamp.any()
