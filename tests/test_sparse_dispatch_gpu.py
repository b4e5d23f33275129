"""The whole dispatch surface of ``ops.emb_bwd_sparse`` vs the CPU ops.

Every (deep rule, wide rule) the entry point takes, each side alone
included, at a deep dim on the quad map (16) and one off it (12: the
one-lane-per-row kernels, and a pair must fall back to the two singles).
Inputs, comparison helper and tolerance are those of
``test_sparse_ftrl_gpu.py`` (exact gradient sums, ``allclose(atol=1e-5)``).
FTRL sides run at ``l1 = 0``: the subject is routing, and without the
exact-zero threshold no element needs to be set aside."""

import pytest
import torch

import test_sparse_ftrl_gpu as ftrl_gpu
import test_sparse_rowwise_adagrad_gpu as rowwise_gpu
from tf_yarn_amd import ops

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X"),
]

LR, WIDE_LR, L2 = ftrl_gpu.LR, ftrl_gpu.WIDE_LR, ftrl_gpu.L2
ROWS, DISTINCT, BATCH, G_DIV = 50, 12, 10, 4
RULES = ["adagrad", "ftrl", "rowwise_adagrad"]
# the pairs with a fused deep+wide kernel
FUSED = {("adagrad", "adagrad"), ("adagrad", "ftrl"), ("ftrl", "ftrl"),
         ("rowwise_adagrad", "adagrad"), ("rowwise_adagrad", "ftrl")}
CASES = [(deep, wide, dim) for dim in (16, 12) for deep in RULES
         for wide in (None, "adagrad", "ftrl")] + \
        [(None, "adagrad", 16), (None, "ftrl", 16)]

SINGLE_OPS = {("adagrad", False): ops.emb_bwd_adagrad,
              ("adagrad", True): ops.emb_bwd_adagrad_wide,
              ("ftrl", False): ops.emb_bwd_ftrl,
              ("ftrl", True): ops.emb_bwd_ftrl_wide,
              ("rowwise_adagrad", False): ops.emb_bwd_rowwise_adagrad}


def _tensors(rule, dim, gen):
    """(table, *states) of one side on the CPU."""
    if rule == "ftrl":
        return ftrl_gpu._states(gen, ROWS, dim)
    state_shape = (ROWS,) if rule == "rowwise_adagrad" else (ROWS, dim)
    return (torch.randn(ROWS, dim, generator=gen),
            torch.rand(state_shape, generator=gen))


def _scalars(rule, lr):
    return dict(lr=lr, l1=0.0, l2=L2) if rule == "ftrl" else dict(lr=lr)


def _side(rule, tensors, grad, lr):
    return ops.SparseSide(rule, tensors[0], tuple(tensors[1:]), grad,
                          **_scalars(rule, lr))


def _side_arg(side, acc):
    """The side as ``_C.emb_bwd_sparse`` takes it."""
    return (side.rule, side.table, list(side.states), acc, side.grad,
            side.lr, side.eps, side.l1, side.l2)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("deep_rule,wide_rule,dim", CASES)
def test_every_route_matches_the_cpu_ops(deep_rule, wide_rule, dim, dtype):
    gen = torch.Generator().manual_seed(11)
    n = BATCH * G_DIV
    cpu, lrs = {}, {}
    if deep_rule is not None:
        cpu["deep"], lrs["deep"] = _tensors(deep_rule, dim, gen), LR
    if wide_rule is not None:
        cpu["wide"] = _tensors(wide_rule, 1, gen)
        lrs["wide"] = WIDE_LR if wide_rule == "ftrl" else LR
    rules = dict(deep=deep_rule, wide=wide_rule)
    gpu = {k: [t.cuda() for t in v] for k, v in cpu.items()}
    first = gpu.get("deep", gpu.get("wide"))[0]
    pair = len(cpu) == 2
    ws = ops.SparseWorkspace(first, gpu["wide"][0] if pair else None)
    fused = pair and (deep_rule, wide_rule) in FUSED and dim == 16
    if pair:
        assert ops._C.sparse_pair_fused_ok(deep_rule, wide_rule,
                                           dim) == fused
    for step in range(2):  # the second epoch meets stamps of the first
        # 40 ids over 12 distinct rows: duplicates are certain
        ids = torch.randperm(ROWS, generator=gen)[:DISTINCT][
            torch.randint(0, DISTINCT, (n,), generator=gen)]
        grads = dict(deep=ftrl_gpu._exact_grads(gen, (n, dim), dtype),
                     wide=ftrl_gpu._exact_grads(gen, (BATCH,), dtype))
        if deep_rule == "rowwise_adagrad":
            rowwise_gpu._assert_row_sums_exact(ids, grads["deep"])
        sides = {k: _side(rules[k], gpu[k], grads[k].cuda(), lrs[k])
                 for k in gpu}
        if pair and not fused and step == 0:
            # the entry point itself refuses what the predicate denies
            before = [t.clone() for v in gpu.values() for t in v]
            with pytest.raises(RuntimeError):
                ops._C.emb_bwd_sparse(
                    _side_arg(sides["deep"], ws.acc),
                    _side_arg(sides["wide"], ws.wide_acc), ws.stamp,
                    ids.cuda(), 1, 0.5)
            torch.cuda.synchronize()
            after = [t for v in gpu.values() for t in v]
            assert all(torch.equal(a, b) for a, b in zip(after, before))
            assert not ws.acc.any() and not ws.wide_acc.any()
            assert not ws.stamp.any()
        ops.emb_bwd_sparse(ids.cuda(), scale=0.5, workspace=ws, **sides)
        for k, tensors in cpu.items():
            SINGLE_OPS[rules[k], k == "wide"](
                *tensors, ids, grads[k], scale=0.5,
                **_scalars(rules[k], lrs[k]))
        for k in cpu:
            assert ftrl_gpu._all_close(gpu[k], cpu[k]), (step, k)
        assert not ws.acc.any()
        assert ws.wide_acc is None or not ws.wide_acc.any()
        # one epoch per launch of pass 2: the fused pair and a side alone
        # take one per step, the two-singles fallback two
        assert ws.epoch == (step + 1) * (2 if pair and not fused else 1)


def test_fused_predicate_lists_exactly_the_fused_pairs():
    ok = ops._C.sparse_pair_fused_ok
    for deep in RULES:
        for wide in RULES:
            assert ok(deep, wide, 16) == ((deep, wide) in FUSED), (deep, wide)
            assert not ok(deep, wide, 12), (deep, wide)
    assert sum(ok(d, w, 16) for d in RULES for w in RULES) == 5
