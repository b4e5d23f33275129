"""Lazy (sparse) Adam HIP kernels vs the CPU op.

Inputs and tolerance are those ``test_sparse_ftrl_gpu.py`` established:
gradients are its ``_exact_grads`` (integers / 8, exact in bf16 and fp32,
every partial sum exact, so atomic arrival order cannot move the summed
gradient), and every tensor is compared with ``torch.allclose(atol=1e-5)``
(rtol 1e-5) against the CPU op, which ``test_sparse_lazy_adam.py`` holds to
a float64 statement of the rule.  What is left between GPU and CPU is the
rounding of one multiply-add per moment, one ``sqrt`` and one division: an
fp32 evaluation of the rule on such inputs differs from float64 by at most
2.4e-7 over three steps.

States: ``m ~ 0.1 * N(0, 1)``, ``v ~ U(0, 0.1)``, with a block of fresh rows
``m = v = 0``; ``eps = 1e-3``, ``beta2 = 0.99``, ``t = 3`` unless a test says
otherwise.  With these a kernel that drops a bias correction or puts
``eps`` inside the root misses by far more than the tolerance
(``test_sparse_lazy_adam.py`` shows both on the CPU)."""

import collections

import pytest
import torch

from test_sparse_ftrl_gpu import _all_close, _close, _exact_grads
from tf_yarn_amd import ops
from tf_yarn_amd.models.synthetic import synthetic_criteo_batch
from tf_yarn_amd.models.wide_deep import WideAndDeep

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X"),
]

LR, WIDE_LR = 0.05, 0.5
BETA1, BETA2, EPS, STEP = 0.9, 0.99, 1e-3, 3
L1, L2 = 0.0, 0.25  # FTRL companions: routing is the subject, no threshold
KW = dict(lr=LR, beta1=BETA1, beta2=BETA2, eps=EPS)


def _states(gen, rows, dim):
    """table, exp_avg, exp_avg_sq; the first quarter of the rows is fresh."""
    w = torch.randn(rows, dim, generator=gen)
    m = torch.randn(rows, dim, generator=gen) * 0.1
    v = torch.rand(rows, dim, generator=gen) * 0.1
    fresh = max(1, rows // 4)
    m[:fresh] = 0
    v[:fresh] = 0
    return w, m, v


def _case(rows, dim, n, dtype, seed, id_hi=None):
    gen = torch.Generator().manual_seed(seed)
    cpu = _states(gen, rows, dim)
    ids = torch.randint(0, id_hi or rows, (n,), generator=gen)
    grad = _exact_grads(gen, (n, dim), dtype)
    return cpu, ids, grad


def _run_both(cpu, ids, grad, step=STEP, scale=1.0, workspace=None):
    """Apply on GPU copies (returned) and in place on the CPU tensors."""
    gpu = [t.cuda() for t in cpu]
    ws = workspace or ops.SparseWorkspace(gpu[0])
    ops.emb_bwd_lazy_adam(*gpu, ids.cuda(), grad.cuda(), step=step,
                          scale=scale, workspace=ws, **KW)
    ops.emb_bwd_lazy_adam(*cpu, ids, grad, step=step, scale=scale, **KW)
    return gpu, ws


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("n", [1000, 1001])
@pytest.mark.parametrize("dim", [16, 4, 64, 256, 1, 7, 12])
def test_apply_matches_reference(dim, n, dtype):
    cpu, ids, grad = _case(500, dim, n, dtype, seed=dim * 7 + n)
    gpu, ws = _run_both(cpu, ids, grad, scale=0.5)
    assert _all_close(gpu, cpu)
    assert not ws.acc.any()


def test_heavy_collisions():
    cpu, ids, grad = _case(8, 16, 4096, torch.float32, seed=1, id_hi=3)
    start = [t.clone() for t in cpu]
    gpu, _ = _run_both(cpu, ids, grad)
    assert _all_close(gpu, cpu)
    for g, s in zip(gpu, start):  # table and both states
        assert torch.equal(g.cpu()[3:], s[3:])


def test_grid_stride_loop_iterates():
    # n * dim/4 = 2.4M quads > 8192 blocks * 256 threads: a second trip,
    # and its last wave is part-filled
    cpu, ids, grad = _case(100_000, 16, 600_000, torch.bfloat16, seed=3)
    gpu, ws = _run_both(cpu, ids, grad)
    assert _all_close(gpu, cpu)
    assert not ws.acc.any()


@pytest.mark.parametrize("dim", [16, 1, 12])
def test_three_steps_on_one_workspace(dim):
    gen = torch.Generator().manual_seed(4)
    cpu = _states(gen, 400, dim)
    start = [t.clone() for t in cpu]
    gpu = [t.cuda() for t in cpu]
    ws = ops.SparseWorkspace(gpu[0])
    for step in (1, 2, 3):
        # overlapping ids, even rows only
        ids = torch.randint(0, 100, (777,), generator=gen) * 2
        grad = _exact_grads(gen, (777, dim), torch.float32)
        ops.emb_bwd_lazy_adam(*gpu, ids.cuda(), grad.cuda(), step=step,
                              workspace=ws, **KW)
        ops.emb_bwd_lazy_adam(*cpu, ids, grad, step=step, **KW)
        assert not ws.acc.any(), f"accumulator dirty after step {step}"
        assert ws.epoch == step
        assert _all_close(gpu, cpu), step
    untouched = torch.cat([torch.arange(1, 400, 2), torch.arange(200, 400)])
    for g, s in zip(gpu, start):
        assert torch.equal(g.cpu()[untouched], s[untouched])


def test_the_step_count_reaches_the_kernel():
    """The same inputs at t = 1 and t = 10 differ as the reference
    differs: step_size is formed from the count on every call."""
    out = {}
    for step in (1, 10):
        cpu, ids, grad = _case(500, 16, 1001, torch.float32, seed=12)
        gpu, _ = _run_both(cpu, ids, grad, step=step)
        assert _all_close(gpu, cpu), step
        out[step] = (gpu[0].cpu(), cpu[0])
    gap_cpu = (out[1][1] - out[10][1]).abs().max()
    gap_gpu = (out[1][0] - out[10][0]).abs().max()
    assert gap_cpu > 1e-3 and gap_gpu > 1e-3  # far outside the tolerance


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_wide_companion(dtype):
    gen = torch.Generator().manual_seed(5)
    f, b = 26, 77
    cpu = _states(gen, 500, 1)
    ids = torch.randint(0, 500, (b, f), generator=gen)
    gw = _exact_grads(gen, (b,), dtype)
    gpu = [t.cuda() for t in cpu]
    ws = ops.SparseWorkspace(gpu[0])
    ops.emb_bwd_lazy_adam_wide(*gpu, ids.cuda(), gw.cuda(), step=STEP,
                               scale=0.5, workspace=ws, **KW)
    ops.emb_bwd_lazy_adam_wide(*cpu, ids, gw, step=STEP, scale=0.5, **KW)
    assert _all_close(gpu, cpu)
    assert not ws.acc.any()


# ---- pairs ------------------------------------------------------------------

def _tensors(rule, dim, gen, rows=500):
    """(table, *states) of one side on the CPU."""
    if rule == "lazy_adam":
        return _states(gen, rows, dim)
    if rule == "ftrl":
        return (torch.randn(rows, dim, generator=gen),
                torch.rand(rows, dim, generator=gen) + 0.1,
                torch.randn(rows, dim, generator=gen) * 0.1)
    return (torch.randn(rows, dim, generator=gen),
            torch.rand(rows, dim, generator=gen))  # adagrad


def _side(rule, tensors, grad, lr, step=STEP):
    if rule == "lazy_adam":
        return ops.SparseSide(rule, tensors[0], tuple(tensors[1:]), grad, lr,
                              EPS, beta1=BETA1, beta2=BETA2, step=step)
    return ops.SparseSide(rule, tensors[0], tuple(tensors[1:]), grad, lr,
                          l1=L1, l2=L2)


def _side_arg(side, acc):
    """The side as ``_C.emb_bwd_sparse`` takes it."""
    arg = (side.rule, side.table, list(side.states), acc, side.grad,
           side.lr, side.eps, side.l1, side.l2)
    if side.rule == "lazy_adam":
        arg += (side.beta1, side.beta2, side.step)
    return arg


def _pair_case(deep_rule, wide_rule, dim, seed=6):
    gen = torch.Generator().manual_seed(seed)
    b, g_div = 41, 26
    n = b * g_div
    deep = _tensors(deep_rule, dim, gen)
    wide = _tensors(wide_rule, 1, gen)
    ids = torch.randint(0, 500, (n,), generator=gen)
    grad = _exact_grads(gen, (n, dim), torch.bfloat16)
    gw = _exact_grads(gen, (b,), torch.bfloat16)
    return deep, wide, ids, grad, gw


@pytest.mark.parametrize("wide_rule", ["lazy_adam", "ftrl"])
def test_fused_pairs_run_as_one_launch(wide_rule):
    assert ops._C.sparse_pair_fused_ok("lazy_adam", wide_rule, 16)
    deep, wide, ids, grad, gw = _pair_case("lazy_adam", wide_rule, 16)
    alone = [t.cuda() for t in deep]
    dev_d, dev_w = [t.cuda() for t in deep], [t.cuda() for t in wide]
    ws = ops.SparseWorkspace(dev_d[0], dev_w[0])
    for call in (1, 2):  # second call: stamps of the first must not block
        step = STEP + call - 1
        ops.emb_bwd_sparse(
            ids.cuda(), scale=0.5, workspace=ws,
            deep=_side("lazy_adam", dev_d, grad.cuda(), LR, step),
            wide=_side(wide_rule, dev_w, gw.cuda(), WIDE_LR, step))
        assert ws.epoch == call
        ops.emb_bwd_sparse(ids, scale=0.5,
                           deep=_side("lazy_adam", deep, grad, LR, step),
                           wide=_side(wide_rule, wide, gw, WIDE_LR, step))
        # the same update on the deep table alone gives the same bits
        ops.emb_bwd_sparse(ids.cuda(), scale=0.5,
                           deep=_side("lazy_adam", alone, grad.cuda(), LR,
                                      step))
    assert _all_close(dev_d + dev_w, deep + wide)
    for a, b in zip(dev_d, alone):
        assert torch.equal(a, b)
    assert not ws.acc.any() and not ws.wide_acc.any()


def test_public_pair_wrappers_match_the_cpu():
    deep, wide, ids, grad, gw = _pair_case("lazy_adam", "lazy_adam", 16, 8)
    dev = [t.cuda() for t in deep + wide]
    ws = ops.SparseWorkspace(dev[0], dev[3])
    ops.emb_bwd_lazy_adam_fused_wide(
        *dev, ids.cuda(), grad.cuda(), gw.cuda(), step=STEP, wide_step=2,
        wide_lr=WIDE_LR, scale=0.5, workspace=ws, **KW)
    ops.emb_bwd_lazy_adam_fused_wide(
        *deep, *wide, ids, grad, gw, step=STEP, wide_step=2, wide_lr=WIDE_LR,
        scale=0.5, **KW)
    assert _all_close(dev, deep + wide) and ws.epoch == 1
    deep, wide, ids, grad, gw = _pair_case("lazy_adam", "ftrl", 16, 9)
    dev = [t.cuda() for t in deep + wide]
    ws = ops.SparseWorkspace(dev[0], dev[3])
    ops.emb_bwd_lazy_adam_ftrl_fused_wide(
        *dev, ids.cuda(), grad.cuda(), gw.cuda(), step=STEP, wide_lr=WIDE_LR,
        l2=L2, scale=0.5, workspace=ws, **KW)
    ops.emb_bwd_lazy_adam_ftrl_fused_wide(
        *deep, *wide, ids, grad, gw, step=STEP, wide_lr=WIDE_LR, l2=L2,
        scale=0.5, **KW)
    assert _all_close(dev, deep + wide) and ws.epoch == 1


@pytest.mark.parametrize("deep_rule,wide_rule,dim", [
    ("lazy_adam", "adagrad", 16), ("adagrad", "lazy_adam", 16),
    ("ftrl", "lazy_adam", 16), ("lazy_adam", "lazy_adam", 12),
    ("lazy_adam", "ftrl", 12)])
def test_pairs_without_a_fused_kernel_take_two_singles(deep_rule, wide_rule,
                                                       dim):
    assert not ops._C.sparse_pair_fused_ok(deep_rule, wide_rule, dim)
    deep, wide, ids, grad, gw = _pair_case(deep_rule, wide_rule, dim, 10)
    dev_d, dev_w = [t.cuda() for t in deep], [t.cuda() for t in wide]
    ws = ops.SparseWorkspace(dev_d[0], dev_w[0])
    # an Adagrad wide side shares the deep side's lr
    wide_lr = LR if wide_rule == "adagrad" else WIDE_LR
    sides = dict(deep=_side(deep_rule, dev_d, grad.cuda(), LR),
                 wide=_side(wide_rule, dev_w, gw.cuda(), wide_lr))
    # the entry point itself refuses what the predicate denies
    before = [t.clone() for t in dev_d + dev_w]
    with pytest.raises(RuntimeError):
        ops._C.emb_bwd_sparse(_side_arg(sides["deep"], ws.acc),
                              _side_arg(sides["wide"], ws.wide_acc),
                              ws.stamp, ids.cuda(), 1, 0.5)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(dev_d + dev_w, before))
    assert not ws.acc.any() and not ws.wide_acc.any()
    assert not ws.stamp.any()
    ops.emb_bwd_sparse(ids.cuda(), scale=0.5, workspace=ws, **sides)
    assert ws.epoch == 2
    ops.emb_bwd_sparse(ids, scale=0.5,
                       deep=_side(deep_rule, deep, grad, LR),
                       wide=_side(wide_rule, wide, gw, wide_lr))
    assert _all_close(dev_d + dev_w, deep + wide)
    assert not ws.acc.any() and not ws.wide_acc.any()


# ---- the entry point --------------------------------------------------------

def test_pass_two_alone_applies_what_the_accumulator_holds():
    cpu, ids, grad = _case(500, 16, 1001, torch.float32, seed=13)
    gpu = [t.cuda() for t in cpu]
    ws = ops.SparseWorkspace(gpu[0])
    # what pass 1 would have left: scale * the summed gradient rows
    ws.acc.index_add_(0, ids.cuda(), grad.cuda() * 0.5)
    ops._C.emb_bwd_sparse(
        ("lazy_adam", gpu[0], gpu[1:], ws.acc, None, LR, EPS, 0.0, 0.0,
         BETA1, BETA2, STEP), None, ws.stamp, ids.cuda(), ws.next_epoch(),
        1.0)
    ops.emb_bwd_lazy_adam(*cpu, ids, grad, step=STEP, scale=0.5, **KW)
    assert _all_close(gpu, cpu)
    assert not ws.acc.any()


def test_bad_sides_raise_before_any_launch():
    table = torch.randn(50, 16).cuda()
    m, v = torch.zeros(50, 16).cuda(), torch.zeros(50, 16).cuda()
    ids = torch.randint(0, 50, (40,)).cuda()
    grad = torch.ones(40, 16).cuda()
    ws = ops.SparseWorkspace(table)
    t0 = table.clone()

    def call(rule="lazy_adam", states=(m, v), lr=LR, eps=EPS,
             tail=(BETA1, BETA2, 1)):
        ops._C.emb_bwd_sparse(
            (rule, table, list(states), ws.acc, grad, lr, eps, 0.0, 0.0)
            + tuple(tail), None, ws.stamp, ids, 1, 1.0)

    bad = [
        dict(tail=()),                       # 9 elements: no betas, no step
        dict(tail=(BETA1, BETA2)),           # 11 elements
        dict(tail=(BETA1, BETA2, 0)),        # step 0
        dict(tail=(BETA1, BETA2, -3)),
        dict(tail=(1.0, BETA2, 1)), dict(tail=(-0.1, BETA2, 1)),
        dict(tail=(BETA1, 1.0, 1)), dict(tail=(BETA1, 1.5, 1)),
        dict(lr=0.0), dict(lr=-1.0), dict(eps=-1e-3),
        dict(states=(m,)),                   # one state short
        dict(states=(m, v[:49].contiguous())),
        dict(rule="adagrad", states=(m,)),   # extra elements on another rule
        dict(rule="ftrl"),
    ]
    for kw in bad:
        with pytest.raises((RuntimeError, TypeError)):
            call(**kw)
    for kw in (dict(step=0), dict(step=1, lr=0.0), dict(step=1, beta2=1.0)):
        with pytest.raises(ValueError):
            ops.emb_bwd_lazy_adam(table, m, v, ids, grad, workspace=ws,
                                  **dict(KW, **kw))
    assert ws.epoch == 0
    wide = torch.zeros(50, 1).cuda()
    wm, wv = torch.zeros_like(wide), torch.zeros_like(wide)
    wws = ops.SparseWorkspace(table, wide)
    gw = torch.ones(10).cuda()
    with pytest.raises(RuntimeError):  # step 0 on the wide side of a pair
        ops._C.emb_bwd_sparse(
            ("lazy_adam", table, [m, v], wws.acc, grad, LR, EPS, 0.0, 0.0,
             BETA1, BETA2, 1),
            ("lazy_adam", wide, [wm, wv], wws.wide_acc, gw, LR, EPS, 0.0,
             0.0, BETA1, BETA2, 0), wws.stamp, ids, 1, 1.0)
    torch.cuda.synchronize()
    assert torch.equal(table, t0) and not m.any() and not v.any()
    assert not ws.acc.any() and not ws.stamp.any()
    assert not wws.acc.any() and not wws.wide_acc.any()
    assert not wws.stamp.any() and not wide.any() and not wm.any()
    call()  # and the good call goes through
    torch.cuda.synchronize()
    assert not torch.equal(table, t0)


# ---- the model --------------------------------------------------------------

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
                        sharded=sharded, sparse_optimizer="lazy_adam",
                        sparse_eps=EPS, sparse_betas=(BETA1, BETA2),
                        wide_sparse_lr=WIDE_LR).cuda()
    counted = _Counted(ops._C.emb_bwd_sparse)
    monkeypatch.setattr(ops._C, "emb_bwd_sparse", counted)
    if sharded:
        e = model.embeddings
        params = (e.weight, e.adam_exp_avg, e.adam_exp_avg_sq,
                  e.wide_weight, e.wide_adam_exp_avg, e.wide_adam_exp_avg_sq)
        sinks = (e._deep_sink, e._wide_sink)
    else:
        d, w = model.deep_embedding, model.wide_embedding
        params = (d.weight, d.adam_exp_avg, d.adam_exp_avg_sq, w.weight,
                  w.adam_exp_avg, w.adam_exp_avg_sq)
        sinks = (d.pending_grads(), w.pending_grads())
    for step in (1, 2, 3):
        dense, ids, labels = synthetic_criteo_batch(
            256, tables, device="cuda", seed=step)
        model(dense, ids % 12, labels=labels).backward()
        (d_ids, d_grad), = [(i.cpu(), g.float().cpu()) for i, g in sinks[0]]
        (w_ids, w_grad), = [(i.cpu(), g.float().cpu()) for i, g in sinks[1]]
        want = [p.detach().cpu().clone() for p in params]
        model.apply_sparse_updates(LR)
        ops.emb_bwd_lazy_adam(*want[:3], d_ids,
                              d_grad.reshape(d_ids.numel(), -1), step=step,
                              **KW)
        ops.emb_bwd_lazy_adam_wide(*want[3:], w_ids, w_grad, step=step,
                                   **dict(KW, lr=WIDE_LR))
        for got, ref in zip(params, want):
            assert _close(got.detach(), ref), step
    if sharded:
        assert counted.calls == {("lazy_adam", "lazy_adam"): 3}
    else:
        assert counted.calls == {("lazy_adam", None): 3,
                                 (None, "lazy_adam"): 3}
    sd = model.state_dict()
    steps = [v for k, v in sd.items() if k.endswith("adam_step")]
    assert len(steps) == 2
    assert all(s.is_cuda and s.dtype == torch.int64 and int(s) == 3
               for s in steps)
    big = [(name, buf) for name, buf in model.named_buffers()
           if "adam" in name or "_adagrad" in name]
    assert len(big) >= 8
    for name, buf in big:
        assert buf.is_cuda and getattr(buf, "_miyarn_sharded", False), name
