"""Sparse FTRL HIP kernels (and the dense ``fused_ftrl``) vs the CPU ops.

Input recipe of ``test_sparse_adagrad_gpu.py``: gradients are
``randint(-32, 33) / 8``, exact in bf16 and fp32 with every partial sum a
multiple of 1/16 far below 2^24/16, so atomic arrival order cannot move
the summed gradient.  States are a positive ``n`` and a small random
``z``.  What is left between GPU and CPU is FMA contraction and sqrt/div
rounding; the tolerance is the project's ``torch.allclose(atol=1e-5)``
(rtol 1e-5), as in the dense and sparse Adagrad GPU tests.  The fp32 CPU
op itself sits within 2.8e-7 (w), 7.7e-6 (z, |z| up to 53) and 5e-8
relative (n) of a float64 evaluation at these shapes
(``test_sparse_ftrl.py``), well inside that bound.

Where ``l1 > 0`` the exactly-zero weights must be the same set on both
sides, except for elements whose ``| |z'| - l1 |`` is below 1e-4 on the
CPU (the weight is continuous through 0 there); at most 1% of the touched
elements may be excused this way, asserted on the reference."""

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


def _close(gpu, cpu):
    return torch.allclose(gpu.cpu(), cpu, atol=1e-5)


def _all_close(gpu_tensors, cpu_tensors):
    return all(_close(g, c) for g, c in zip(gpu_tensors, cpu_tensors))


def _zeros_agree(w_gpu, w_cpu, z_cpu, ids, l1):
    """Same exact-zero set on the touched rows, away from the threshold;
    the excused share is capped on the reference."""
    rows = torch.unique(ids.reshape(-1))
    sure = ((z_cpu[rows].abs() - l1).abs() >= Z_MARGIN)
    assert float((~sure).double().mean()) <= 0.01
    got, want = (w_gpu.cpu()[rows] == 0.0), (w_cpu[rows] == 0.0)
    return torch.equal(got[sure], want[sure])


def _exact_grads(gen, shape, dtype):
    g = torch.randint(-32, 33, shape, generator=gen).float() / 8
    return g.to(dtype)


def _states(gen, rows, dim):
    """table, accum (positive), linear (small)."""
    return (torch.randn(rows, dim, generator=gen),
            torch.rand(rows, dim, generator=gen) + 0.1,
            torch.randn(rows, dim, generator=gen) * 0.1)


def _case(rows, dim, n, dtype, seed, id_hi=None):
    gen = torch.Generator().manual_seed(seed)
    cpu = _states(gen, rows, dim)
    ids = torch.randint(0, id_hi or rows, (n,), generator=gen)
    grad = _exact_grads(gen, (n, dim), dtype)
    return cpu, ids, grad


def _run_both(cpu, ids, grad, scale=1.0, l1=L1, l2=L2, workspace=None):
    """Apply on GPU copies (returned) and in place on the CPU tensors."""
    gpu = [t.cuda() for t in cpu]
    ws = workspace or ops.SparseWorkspace(gpu[0])
    ops.emb_bwd_ftrl(*gpu, ids.cuda(), grad.cuda(), lr=LR, l1=l1, l2=l2,
                     scale=scale, workspace=ws)
    ops.emb_bwd_ftrl(*cpu, ids, grad, lr=LR, l1=l1, l2=l2, scale=scale)
    return gpu, ws


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("n", [1000, 1001])
@pytest.mark.parametrize("dim", [16, 4, 64, 1, 7, 12])
def test_apply_matches_reference(dim, n, dtype):
    cpu, ids, grad = _case(500, dim, n, dtype, seed=dim * 7 + n)
    gpu, ws = _run_both(cpu, ids, grad, scale=0.5)
    assert _all_close(gpu, cpu)
    assert _zeros_agree(gpu[0], cpu[0], cpu[2], ids, L1)
    assert not ws.acc.any()


def test_no_regularisation():
    cpu, ids, grad = _case(500, 16, 1001, torch.float32, seed=9)
    gpu, _ = _run_both(cpu, ids, grad, scale=0.5, l1=0.0, l2=0.0)
    assert _all_close(gpu, cpu)


def test_heavy_collisions():
    cpu, ids, grad = _case(8, 16, 4096, torch.float32, seed=1, id_hi=3)
    t0 = cpu[0].clone()
    gpu, _ = _run_both(cpu, ids, grad)
    assert _all_close(gpu, cpu)
    assert torch.equal(gpu[0].cpu()[3:], t0[3:])


def test_many_rows_per_wave():
    cpu, ids, grad = _case(64, 4, 4096, torch.bfloat16, seed=2)
    gpu, _ = _run_both(cpu, ids, grad)
    assert _all_close(gpu, cpu)
    assert _zeros_agree(gpu[0], cpu[0], cpu[2], ids, L1)


def test_grid_stride_loop_iterates():
    # n * dim/4 = 2.4M quads > 8192 blocks * 256 threads
    cpu, ids, grad = _case(100_000, 16, 600_000, torch.bfloat16, seed=3)
    gpu, ws = _run_both(cpu, ids, grad)
    assert _all_close(gpu, cpu)
    assert _zeros_agree(gpu[0], cpu[0], cpu[2], ids, L1)
    assert not ws.acc.any()


@pytest.mark.parametrize("dim", [16, 1, 12])
def test_three_steps_on_one_workspace(dim):
    gen = torch.Generator().manual_seed(4)
    cpu = _states(gen, 400, dim)
    start = [t.clone() for t in cpu]
    gpu = [t.cuda() for t in cpu]
    ws = ops.SparseWorkspace(gpu[0])
    for step in range(3):
        # overlapping ids, even rows only
        ids = torch.randint(0, 100, (777,), generator=gen) * 2
        grad = _exact_grads(gen, (777, dim), torch.float32)
        ops.emb_bwd_ftrl(*gpu, ids.cuda(), grad.cuda(), lr=LR, l1=L1,
                         l2=L2, workspace=ws)
        ops.emb_bwd_ftrl(*cpu, ids, grad, lr=LR, l1=L1, l2=L2)
        assert not ws.acc.any(), f"accumulator dirty after step {step}"
        assert ws.epoch == step + 1
        assert _all_close(gpu, cpu), step
        assert _zeros_agree(gpu[0], cpu[0], cpu[2], ids, L1), step
    untouched = torch.cat([torch.arange(1, 400, 2), torch.arange(200, 400)])
    for g, s in zip(gpu, start):
        assert torch.equal(g.cpu()[untouched], s[untouched])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_wide_companion(dtype):
    gen = torch.Generator().manual_seed(5)
    f, b = 26, 77
    cpu = _states(gen, 500, 1)
    ids = torch.randint(0, 500, (b, f), generator=gen)
    gw = _exact_grads(gen, (b,), dtype)
    gpu = [t.cuda() for t in cpu]
    ws = ops.SparseWorkspace(gpu[0])
    ops.emb_bwd_ftrl_wide(*gpu, ids.cuda(), gw.cuda(), lr=LR, l1=L1, l2=L2,
                          scale=0.5, workspace=ws)
    ops.emb_bwd_ftrl_wide(*cpu, ids, gw, lr=LR, l1=L1, l2=L2, scale=0.5)
    assert _all_close(gpu, cpu)
    assert _zeros_agree(gpu[0], cpu[0], cpu[2], ids, L1)
    assert not ws.acc.any()


# dim 12 and mixed grad dtypes take the two single-table kernels
@pytest.mark.parametrize("dim,mixed", [(16, False), (64, False),
                                       (12, False), (16, True)])
@pytest.mark.parametrize("g_div", [4, 26])
@pytest.mark.parametrize("deep_rule", ["adagrad", "ftrl"])
def test_fused_deep_wide(deep_rule, g_div, dim, mixed):
    gen = torch.Generator().manual_seed(6 + g_div)
    rows, b = 500, 41
    n = b * g_div
    deep = _states(gen, rows, dim)
    if deep_rule == "adagrad":
        deep = deep[:2]  # table, state_sum
    wide = _states(gen, rows, 1)
    ids = torch.randint(0, rows, (n,), generator=gen)
    grad = _exact_grads(gen, (n, dim), torch.bfloat16)
    gw = _exact_grads(gen, (b,),
                      torch.float32 if mixed else torch.bfloat16)
    dev = [t.cuda() for t in deep + wide]
    ws = ops.SparseWorkspace(dev[0], dev[len(deep)])
    for _ in range(2):  # second call: stamps of the first must not block
        if deep_rule == "adagrad":
            ops.emb_bwd_adagrad_ftrl_fused_wide(
                *dev, ids.cuda(), grad.cuda(), gw.cuda(), lr=LR,
                wide_lr=WIDE_LR, l1=L1, l2=L2, scale=0.5, workspace=ws)
            ops.emb_bwd_adagrad(*deep, ids, grad, lr=LR, scale=0.5)
        else:
            ops.emb_bwd_ftrl_fused_wide(
                *dev, ids.cuda(), grad.cuda(), gw.cuda(), lr=LR,
                wide_lr=WIDE_LR, l1=L1, l2=L2, scale=0.5, workspace=ws)
            ops.emb_bwd_ftrl(*deep, ids, grad, lr=LR, l1=L1, l2=L2,
                             scale=0.5)
        ops.emb_bwd_ftrl_wide(*wide, ids, gw, lr=WIDE_LR, l1=L1, l2=L2,
                              scale=0.5)
    assert _all_close(dev, deep + wide)
    w_gpu, w_cpu = dev[len(deep)], wide[0]
    assert _zeros_agree(w_gpu, w_cpu, wide[2], ids, L1)
    assert not ws.acc.any() and not ws.wide_acc.any()
    assert ws.epoch == (2 if dim != 12 and not mixed else 4)


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
    l1, l2 = 0.001, 0.01
    model = WideAndDeep(table_sizes=tables, embedding_dim=16,
                        hidden=(64, 32), compute_dtype=torch.bfloat16,
                        sharded=sharded, sparse_optimizer="adagrad",
                        wide_sparse_optimizer="ftrl", sparse_l1=l1,
                        sparse_l2=l2, wide_sparse_lr=WIDE_LR,
                        sparse_initial_accumulator=0.1).cuda()
    counted = _Counted(ops._C.emb_bwd_sparse)
    monkeypatch.setattr(ops._C, "emb_bwd_sparse", counted)
    if sharded:
        e = model.embeddings
        params = (e.weight, e.state_sum, e.wide_weight, e.wide_ftrl_accum,
                  e.wide_ftrl_linear)
        sinks = (e._deep_sink, e._wide_sink)
    else:
        d, w = model.deep_embedding, model.wide_embedding
        params = (d.weight, d.state_sum, w.weight, w.ftrl_accum,
                  w.ftrl_linear)
        sinks = (d.pending_grads(), w.pending_grads())
    for step in range(2):
        dense, ids, labels = synthetic_criteo_batch(
            256, tables, device="cuda", seed=step)
        model(dense, ids % 12, labels=labels).backward()
        (d_ids, d_grad), = [(i.cpu(), g.float().cpu()) for i, g in sinks[0]]
        (w_ids, w_grad), = [(i.cpu(), g.float().cpu()) for i, g in sinks[1]]
        dt, ds, wt, wn, wz = [p.detach().cpu().clone() for p in params]
        model.apply_sparse_updates(LR)
        ops.emb_bwd_adagrad(dt, ds, d_ids,
                            d_grad.reshape(d_ids.numel(), -1), lr=LR)
        ops.emb_bwd_ftrl_wide(wt, wn, wz, w_ids, w_grad, lr=WIDE_LR, l1=l1,
                              l2=l2)
        for got, want in zip(params, (dt, ds, wt, wn, wz)):
            assert _close(got.detach(), want), step
    if sharded:
        assert counted.calls == {("adagrad", "ftrl"): 2}
    else:
        assert counted.calls == {("adagrad", None): 2, (None, "ftrl"): 2}
    big = [(name, buf) for name, buf in model.named_buffers()
           if "state_sum" in name or "ftrl" in name or "_adagrad" in name]
    assert len(big) >= 6
    for name, buf in big:
        assert buf.is_cuda and getattr(buf, "_miyarn_sharded", False), name


def _ftrl_side(table, accum, linear, acc, grad, lr=LR, l1=0.0, l2=0.0):
    """An FTRL side as ``_C.emb_bwd_sparse`` takes it (``grad=None``: pass
    2 alone)."""
    return ("ftrl", table, [accum, linear], acc, grad, lr, 1e-10, l1, l2)


def test_bad_inputs_raise_before_any_launch():
    table = torch.randn(50, 16).cuda()
    accum = torch.ones(50, 16).cuda()
    linear = torch.zeros(50, 16).cuda()
    ids = torch.randint(0, 50, (40,)).cuda()
    grad = torch.ones(40, 16).cuda()
    ws = ops.SparseWorkspace(table)
    t0 = table.clone()

    def call(table=table, accum=accum, linear=linear, acc=ws.acc,
             stamp=ws.stamp, ids=ids, grad=grad, lr=LR, l1=0.0, l2=0.0):
        ops._C.emb_bwd_sparse(
            _ftrl_side(table, accum, linear, acc, grad, lr, l1, l2), None,
            stamp, ids, 1, 1.0)

    bad = [
        dict(grad=grad.half()),                       # dtype
        dict(grad=grad.t().contiguous().t()),         # non-contiguous
        dict(grad=grad[:39].contiguous()),            # shape
        dict(accum=accum.double()),
        dict(accum=accum[:49].contiguous()),
        dict(linear=linear.double()),
        dict(linear=torch.zeros(16, 50).cuda().t()),
        dict(linear=linear[:49].contiguous()),
        dict(linear=None),                            # missing second state
        dict(table=table.t().contiguous().t()),
        dict(acc=ws.acc[:, :8].contiguous()),
        dict(stamp=ws.stamp.long()),
        dict(stamp=ws.stamp[:49].contiguous()),
        dict(ids=ids.int()),
        dict(ids=torch.arange(80).cuda()[::2]),
        dict(l1=-0.1), dict(l2=-0.1), dict(lr=0.0),
    ]
    for kw in bad:
        with pytest.raises((RuntimeError, TypeError)):
            call(**kw)
    for kw in (dict(l1=-0.1), dict(l2=-0.1), dict(lr=0.0)):
        kw = dict(dict(lr=LR), **kw)
        with pytest.raises(ValueError):
            ops.emb_bwd_ftrl(table, accum, linear, ids, grad, workspace=ws,
                             **kw)
    assert ws.epoch == 0
    wide = torch.zeros(50, 1).cuda()
    wn, wz = torch.ones_like(wide), torch.zeros_like(wide)
    wws = ops.SparseWorkspace(table, wide)
    bf16_gw = torch.ones(10, dtype=torch.bfloat16).cuda()
    gw = torch.ones(10).cuda()
    with pytest.raises(RuntimeError):  # gw dtype differs from grad's
        ops._C.emb_bwd_sparse(
            ("adagrad", table, [accum], wws.acc, grad, LR, 1e-10, 0.0, 0.0),
            _ftrl_side(wide, wn, wz, wws.wide_acc, bf16_gw),
            wws.stamp, ids, 1, 1.0)
    with pytest.raises(RuntimeError):  # wide linear is deep-shaped
        ops._C.emb_bwd_sparse(
            _ftrl_side(table, accum, linear, wws.acc, grad),
            _ftrl_side(wide, wn, linear, wws.wide_acc, gw),
            wws.stamp, ids, 1, 1.0)
    with pytest.raises(RuntimeError):  # negative l1 on the fused entry
        ops._C.emb_bwd_sparse(
            _ftrl_side(table, accum, linear, wws.acc, grad, l1=-1.0),
            _ftrl_side(wide, wn, wz, wws.wide_acc, gw, l1=-1.0),
            wws.stamp, ids, 1, 1.0)
    with pytest.raises(RuntimeError):  # 40 ids, 7 examples
        ops._C.emb_bwd_sparse(
            None, _ftrl_side(wide, wn, wz, wws.wide_acc,
                             torch.ones(7).cuda()),
            wws.stamp, ids, 1, 1.0)
    with pytest.raises(RuntimeError):  # pass 2 alone checks too
        ops._C.emb_bwd_sparse(
            _ftrl_side(table, accum, linear[:49].contiguous(), ws.acc, None),
            None, ws.stamp, ids, 1, 1.0)
    torch.cuda.synchronize()
    assert torch.equal(table, t0)
    assert torch.equal(accum, torch.ones_like(accum))
    assert not linear.any() and not ws.acc.any() and not ws.stamp.any()
    assert not wws.acc.any() and not wws.wide_acc.any()
    assert not wws.stamp.any() and not wz.any() and not wide.any()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_dense_fused_ftrl(dtype):
    gen = torch.Generator().manual_seed(8)
    n = 50_001  # odd: the scalar tail runs
    w = torch.randn(n, generator=gen)
    acc = torch.full((n,), 0.1)
    lin = torch.zeros(n)
    gpu = [t.cuda() for t in (w, acc, lin)]
    for step in range(3):
        g = torch.randn(n, generator=gen).to(dtype)
        ops.fused_ftrl(gpu[0], g.cuda(), gpu[1], gpu[2], lr=LR, l1=0.05,
                       l2=L2, grad_scale=0.5)
        ops.fused_ftrl(w, g, acc, lin, lr=LR, l1=0.05, l2=L2,
                       grad_scale=0.5)
        assert _all_close(gpu, (w, acc, lin)), step
    sure = (lin.abs() - 0.05).abs() >= Z_MARGIN
    assert float((~sure).double().mean()) <= 0.01
    assert torch.equal((gpu[0].cpu() == 0.0)[sure], (w == 0.0)[sure])
    assert (w == 0.0).any()
