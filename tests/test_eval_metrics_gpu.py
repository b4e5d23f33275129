"""``binary_eval_update`` on the GPU (csrc/eval_metrics.hip) against the
CPU reference of the same spec (tested on its own in test_eval_metrics.py).

``hist`` and ``counts`` are integers and the bucket expression is one
fp32 rounding on both sides, so they are compared with ``torch.equal``.
The launch is 256 threads x min(ceil(n/256), 256) blocks: the sizes cover
one thread, one block ragged / full / plus one, the full grid plus three
threads on a second trip of the grid-stride loop, and a ragged second trip.

The two fp64 sums are compared at ``RTOL = 1e-5``: device ``expf``,
``log1pf`` and the division are each within a few fp32 ulp, every term is
non-negative for 0/1 labels so the sum inherits about 1e-6 relative, and
fp64 accumulation adds less than n * 2^-53; 1e-5 leaves roughly ten times
that.
"""

import math

import pytest
import torch

from tf_yarn_amd import ops
from tf_yarn_amd.estimator import BinaryClassificationMetrics
from tf_yarn_amd.estimator.eval_metrics import KEYS

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")

F32, BF16 = torch.float32, torch.bfloat16
RTOL = 1e-5
FLOAT_KEYS = ("average_loss", "prediction/mean")
SIZES = [1, 255, 256, 257, 65539, 70001]


def _exact_batch(n, dtype, seed):
    """Logits on a grid that both dtypes hold exactly, spanning [-20, 20]
    so both clamps are hit (fp32: k/64; bf16: k/8, |k| <= 160), the
    special values in front, random 0/1 labels with both classes."""
    g = torch.Generator().manual_seed(seed)
    if dtype == F32:
        z = torch.randint(-1280, 1281, (n,), generator=g).float() / 64.0
    else:
        z = torch.randint(-160, 161, (n,), generator=g).float() / 8.0
    y = (torch.rand(n, generator=g) < 0.35).float()
    nan, inf = float("nan"), float("inf")
    zs = torch.tensor([-16.0, 16.0, 16.0 - 2.0 ** -7, 0.0, -0.0, inf, -inf,
                       -20.0, 20.0, nan, 1.0, nan])
    ys = torch.tensor([1.0, 0.0, 1.0, 1.0, 0.0, 1.0, 0.0,
                       1.0, 0.0, 1.0, nan, nan])
    if n >= len(zs):
        z[:len(zs)] = zs
        y[:len(ys)] = ys
        assert 0 < int((y == 1).sum()) < n
    return z.to(dtype), y


def _states(batches):
    """(GPU state, CPU reference state) after the same batches."""
    dev, ref = ops.BinaryEvalState("cuda"), ops.BinaryEvalState("cpu")
    for z, y in batches:
        ops.binary_eval_update(z.cuda(), y.cuda(), dev)
        ops.binary_eval_update(z, y, ref)
    return dev, ref


def _assert_ints_equal(dev, ref):
    assert torch.equal(dev.hist.cpu(), ref.hist)
    assert torch.equal(dev.counts.cpu(), ref.counts)


@requires_gpu
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("n", SIZES)
def test_state_is_the_reference_exactly(n, dtype):
    z, y = _exact_batch(n, dtype, seed=n)
    dev, ref = _states([(z, y)])
    _assert_ints_equal(dev, ref)
    assert int(dev.counts[0]) + int(dev.counts[1]) == n
    assert int(dev.hist.sum()) == int(dev.counts[0])
    # slots past the grid stay untouched
    grid = min((n + 255) // 256, ops.EVAL_SLOTS)
    assert torch.count_nonzero(dev.sums[grid:]).item() == 0


@requires_gpu
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_calls_accumulate(dtype):
    parts = [_exact_batch(n, dtype, seed=100 + n) for n in (300, 66000, 77)]
    dev, _ = _states(parts)
    whole_z = torch.cat([z for z, _ in parts])
    whole_y = torch.cat([y for _, y in parts])
    one, ref = _states([(whole_z, whole_y)])
    _assert_ints_equal(dev, ref)
    _assert_ints_equal(one, ref)


@requires_gpu
def test_one_bin_takes_every_add():
    z = torch.full((4096,), 0.25)
    y = torch.ones(4096)
    dev, _ = _states([(z, y)])
    want = torch.zeros(2, ops.EVAL_BUCKETS, dtype=torch.int64)
    want[1, 2048 + 32] = 4096
    assert torch.equal(dev.hist.cpu(), want)
    assert dev.counts.tolist() == [4096, 0, 4096, 0]
    m = BinaryClassificationMetrics()
    m.update(z.cuda(), y.cuda())
    assert m.result()["auc"] == 0.0


def _finite_batch(n, seed):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(n, generator=g) * 3.0
    y = (torch.rand(n, generator=g) < 0.3).float()
    return z, y


@requires_gpu
@pytest.mark.parametrize("n", [257, 70001])
def test_float_sums_against_float64(n):
    """Largest relative error seen on an MI355X: 3.2e-9 (docs/Kernels.md)."""
    z, y = _finite_batch(n, seed=n)
    dev = ops.BinaryEvalState("cuda")
    ops.binary_eval_update(z.cuda(), y.cuda(), dev)
    got_loss, got_sig = dev.sums.cpu().sum(dim=0).tolist()
    z64, y64 = z.double(), y.double()
    want_loss = (z64.clamp_min(0) - z64 * y64
                 + torch.log1p(torch.exp(-z64.abs()))).sum().item()
    want_sig = (1.0 / (1.0 + torch.exp(-z64))).sum().item()
    rel_loss = abs(got_loss - want_loss) / want_loss
    rel_sig = abs(got_sig - want_sig) / want_sig
    print(f"n={n} rel err: loss sum {rel_loss:.3e}, sigmoid sum "
          f"{rel_sig:.3e}")
    assert rel_loss <= RTOL
    assert rel_sig <= RTOL


@requires_gpu
def test_same_batches_give_the_same_bits():
    parts = [_finite_batch(n, seed=200 + n) for n in (300, 66000, 77)]
    parts = [(z.cuda(), y.cuda()) for z, y in parts]
    a, b = ops.BinaryEvalState("cuda"), ops.BinaryEvalState("cuda")
    for state in (a, b):
        for z, y in parts:
            ops.binary_eval_update(z, y, state)
    assert torch.equal(a.sums, b.sums)
    assert torch.equal(a.hist, b.hist)
    assert torch.equal(a.counts, b.counts)
    assert torch.count_nonzero(a.sums).item() > 2


@requires_gpu
def test_accumulator_on_gpu_matches_cpu():
    parts = [_finite_batch(n, seed=300 + n) for n in (5000, 66000)]
    dev, cpu = BinaryClassificationMetrics(), BinaryClassificationMetrics()
    for z, y in parts:
        dev.update(z.cuda().reshape(-1, 1), y.cuda())
        cpu.update(z.reshape(-1, 1), y)
    got, want = dev.result(), cpu.result()
    assert set(got) == set(KEYS)
    for k in KEYS:
        if k in FLOAT_KEYS:
            assert got[k] == pytest.approx(want[k], rel=RTOL), k
        else:
            assert got[k] == want[k], k
    assert 0.0 < got["auc"] < 1.0


@requires_gpu
@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "fp32"])
def test_model_logits_feed_the_accumulator(dtype):
    from tf_yarn_amd.models.synthetic import synthetic_criteo_batch
    from tf_yarn_amd.models.wide_deep import WideAndDeep
    tables = [50] * 4
    torch.manual_seed(0)
    model = WideAndDeep(table_sizes=tables, embedding_dim=4, hidden=(8,),
                        compute_dtype=dtype).to("cuda").eval()
    dense, ids, labels = synthetic_criteo_batch(64, tables, device="cuda",
                                                seed=0)
    with torch.no_grad():
        logits = model(dense, ids)
    m = BinaryClassificationMetrics()
    m.update(logits, labels)
    r = m.result()
    assert set(r) == set(KEYS)
    assert all(math.isfinite(v) for v in r.values())
    assert r["examples"] == 64.0 and r["nan_examples"] == 0.0
