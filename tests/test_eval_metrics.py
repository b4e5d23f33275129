"""Streaming binary eval metrics on the CPU: the torch reference of
``ops.binary_eval_update`` (the spec the HIP kernel is tested against in
test_eval_metrics_gpu.py), ``BinaryClassificationMetrics`` on top of it,
and its wiring into ``Estimator.evaluate`` and the Keras shim.

Everything derived from the integer state is compared exactly: the
accumulator works in Python integers with one division at the end, and so
do the brute-force references here.
"""

import logging
import math
from fractions import Fraction

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp
from torch import nn

from tf_yarn_amd import ops
from tf_yarn_amd.estimator import BinaryClassificationMetrics, Estimator
from tf_yarn_amd.estimator.eval_metrics import KEYS
from tf_yarn_amd.estimator.keras import Callback, KerasModel, load_model
from tf_yarn_amd.estimator.metrics import get_all_metrics
from tf_yarn_amd.kv import KVClient, KVServer

FLOAT_KEYS = ("average_loss", "prediction/mean")
INT_KEYS = tuple(k for k in KEYS if k not in FLOAT_KEYS)


def _buckets(z):
    """Bucket index of fp32 logits by the spec, in numpy."""
    t = (z.numpy().astype(np.float32) + np.float32(16.0)) * np.float32(128.0)
    return np.clip(np.floor(t), 0, ops.EVAL_BUCKETS - 1).astype(np.int64)


def _brute_auc(score, y):
    """O(P*N) Mann-Whitney, ties one half; one division of Python ints."""
    pos, neg = score[y >= 0.5], score[y < 0.5]
    wins = int((pos[:, None] > neg[None, :]).sum())
    ties = int((pos[:, None] == neg[None, :]).sum())
    return (2 * wins + ties) / (2 * len(pos) * len(neg))


def _brute_average_precision(k, y):
    """Mean over the positives of the precision at the positive's own
    bucket as threshold, exact in rationals."""
    total = Fraction(0)
    for kp in k[y >= 0.5]:
        above = k >= kp
        total += Fraction(int((above & (y >= 0.5)).sum()), int(above.sum()))
    return total / int((y >= 0.5).sum())


def _random_batch(n, seed, pos_rate=0.3):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(n, generator=g) * 3.0
    y = (torch.rand(n, generator=g) < pos_rate).float()
    return z, y


def _result(z, y):
    m = BinaryClassificationMetrics()
    m.update(z, y)
    return m.result()


# ---- the reference against brute force --------------------------------------

def test_auc_is_the_mann_whitney_of_the_bucketed_scores():
    z, y = _random_batch(5000, seed=0)
    assert _result(z, y)["auc"] == _brute_auc(_buckets(z), y.numpy())


def test_auc_of_one_value_per_bucket_is_the_exact_auc():
    """Distinct multiples of 1/128 inside (-16, 16): every bucket holds one
    distinct value, so bucketing loses nothing."""
    g = torch.Generator().manual_seed(1)
    ks = torch.randperm(4095, generator=g)[:4000] - 2047  # -2047 .. 2047
    z = ks.float() / 128.0
    y = (torch.rand(4000, generator=g) < 0.4).float()
    assert len(set(_buckets(z).tolist())) == 4000
    got = _result(z, y)["auc"]
    assert got == _brute_auc(z.numpy().astype(np.float64), y.numpy())
    assert got == _brute_auc(_buckets(z), y.numpy())


def test_average_precision_against_brute_force():
    """The accumulator rounds once per bucket term (non-negative terms),
    sums them exactly (fsum) and divides once: at most 3 roundings of
    2^-53 relative against the rational value."""
    z, y = _random_batch(3000, seed=2)
    want = float(_brute_average_precision(_buckets(z), y.numpy()))
    got = _result(z, y)["auc_precision_recall"]
    assert abs(got - want) <= 4 * 2.0 ** -53 * want
    assert 0.0 < got < 1.0


def test_confusion_metrics_against_direct_counts():
    z, y = _random_batch(2000, seed=3)
    r = _result(z, y)
    pos, hot = y >= 0.5, z > 0
    tp, fp = int((pos & hot).sum()), int((~pos & hot).sum())
    n, n_pos = 2000, int(pos.sum())
    assert r["accuracy"] == (tp + (n - n_pos) - fp) / n
    assert r["precision"] == tp / (tp + fp)
    assert r["recall"] == tp / n_pos
    assert r["label/mean"] == n_pos / n
    assert r["examples"] == 2000.0 and r["nan_examples"] == 0.0
    z64, y64 = z.double(), y.double()
    loss = (z64.clamp_min(0) - z64 * y64
            + torch.log1p(torch.exp(-z64.abs()))).mean().item()
    assert r["average_loss"] == pytest.approx(loss, rel=1e-6)
    assert r["prediction/mean"] == pytest.approx(
        torch.sigmoid(z64).mean().item(), rel=1e-6)


# ---- bucket edges, NaN, degenerate mixes ------------------------------------

def test_bucket_edges_and_nan():
    nan, inf = float("nan"), float("inf")
    z = torch.tensor([-16.0, 16.0, 16.0 - 2.0 ** -7, 0.0, -0.0, inf, -inf,
                      -16.0 - 2.0 ** -6, nan, 1.0, nan])
    y = torch.tensor([1.0, 0.0, 1.0, 1.0, 0.0, 1.0, 0.0,
                      0.0, 1.0, nan, nan])
    state = ops.BinaryEvalState("cpu")
    ops.binary_eval_update(z, y, state)
    want = torch.zeros(2, ops.EVAL_BUCKETS, dtype=torch.int64)
    want[1, 0] = 1      # -16
    want[0, 4095] = 1   # 16
    want[1, 4095] = 2   # 16 - 2^-7, +inf
    want[1, 2048] = 1   # +0
    want[0, 2048] = 1   # -0
    want[0, 0] = 2      # -inf, just below -16
    assert torch.equal(state.hist, want)
    # (n_valid, n_nan, tp, fp): z > 0 holds for 16 (neg), 16-2^-7 and +inf
    assert state.counts.tolist() == [8, 3, 2, 1]
    m = BinaryClassificationMetrics()
    m.update(z, y)
    r = m.result()
    assert r["examples"] == 8.0 and r["nan_examples"] == 3.0


def test_bf16_and_integer_inputs_are_widened():
    z = torch.tensor([0.5, -2.0, 3.0, -0.25])
    y = torch.tensor([1, 0, 1, 0])
    a, b = ops.BinaryEvalState("cpu"), ops.BinaryEvalState("cpu")
    ops.binary_eval_update(z, y.float(), a)
    ops.binary_eval_update(z.to(torch.bfloat16).reshape(2, 2),
                           y.reshape(2, 2), b)
    for s, t in zip(a.tensors(), b.tensors()):
        assert torch.equal(s, t)
    ops.binary_eval_update(z[:0], y[:0], a)  # empty: no-op
    assert torch.equal(a.hist, b.hist)
    assert b.zero_().hist.sum() == 0 and b.sums.abs().sum() == 0


@pytest.mark.parametrize("label", [0.0, 1.0])
def test_single_class_gives_zero_auc(label):
    z, _ = _random_batch(100, seed=4)
    r = _result(z, torch.full((100,), label))
    assert r["auc"] == 0.0
    assert r["label/mean"] == label
    assert r["auc_precision_recall"] == label  # no positives: 0.0
    assert all(math.isfinite(v) for v in r.values())


def test_empty_accumulator_result():
    r = BinaryClassificationMetrics().result()
    assert set(r) == set(KEYS)
    assert all(v == 0.0 for v in r.values())


# ---- merge, order, all_reduce -----------------------------------------------

def test_merge_and_update_order():
    z, y = _random_batch(4000, seed=5)
    whole = _result(z, y)
    a, b = BinaryClassificationMetrics(), BinaryClassificationMetrics()
    a.update(z[:1500], y[:1500])
    b.update(z[1500:], y[1500:])
    a.merge(b)
    merged = a.result()
    rev = BinaryClassificationMetrics()
    for lo, hi in ((3000, 4000), (0, 700), (700, 3000)):
        rev.update(z[lo:hi].reshape(-1, 1), y[lo:hi])
    reordered = rev.result()
    for k in INT_KEYS:
        assert merged[k] == whole[k], k
        assert reordered[k] == whole[k], k
    for k in FLOAT_KEYS:
        assert merged[k] == pytest.approx(whole[k], rel=1e-12)
        assert reordered[k] == pytest.approx(whole[k], rel=1e-12)
    rev.reset()
    assert rev.result()["examples"] == 0.0


def _all_reduce_worker(rank, world_size, kv_addr, out_q):
    from tf_yarn_amd.parallel import comm
    client = KVClient(kv_addr)
    comm.init_process_group(rank=rank, world_size=world_size,
                            backend="gloo", kv_client=client)
    try:
        z, y = _random_batch(2000, seed=6)
        m = BinaryClassificationMetrics()
        m.update(z[rank::world_size], y[rank::world_size])
        m.all_reduce()
        out_q.put((rank, m.result()))
    finally:
        comm.destroy_process_group()


def test_all_reduce_pools_the_ranks():
    world_size = 2
    server = KVServer()
    ctx = mp.get_context("spawn")
    out_q = ctx.Queue()
    procs = [ctx.Process(target=_all_reduce_worker,
                         args=(r, world_size, server.address, out_q))
             for r in range(world_size)]
    for p in procs:
        p.start()
    try:
        results = dict(out_q.get(timeout=120) for _ in range(world_size))
    finally:
        for p in procs:
            p.join(timeout=30)
            if p.is_alive():
                p.terminate()
        server.stop()
    whole = _result(*_random_batch(2000, seed=6))
    for rank in range(world_size):
        for k in INT_KEYS:
            assert results[rank][k] == whole[k], (rank, k)
        for k in FLOAT_KEYS:
            assert results[rank][k] == pytest.approx(whole[k], rel=1e-12)


def test_all_reduce_without_process_group_is_a_noop():
    z, y = _random_batch(50, seed=7)
    m = BinaryClassificationMetrics()
    m.update(z, y)
    before = m.result()
    m.all_reduce()
    assert m.result() == before


# ---- Estimator --------------------------------------------------------------

# logit == feature.  Each batch ranks perfectly on its own (AUC 1.0 each);
# pooled, the negative at 1.0 outranks the positive at -1.0: 5 of 6 pairs.
_EVAL_BATCHES = [
    (torch.tensor([[2.0], [1.0]]), torch.tensor([1.0, 0.0])),
    (torch.tensor([[-1.0], [-2.0], [-3.0]]), torch.tensor([1.0, 0.0, 0.0])),
]


def _identity_estimator(model_dir, **kwargs):
    def module_fn():
        lin = nn.Linear(1, 1)
        with torch.no_grad():
            lin.weight.fill_(1.0)
            lin.bias.zero_()
        return lin

    def loss_fn(out, labels):
        return nn.functional.binary_cross_entropy_with_logits(
            out.squeeze(-1), labels)

    return Estimator(module_fn, lambda p: torch.optim.SGD(p, lr=0.1),
                     loss_fn, model_dir=model_dir, device="cpu", **kwargs)


def test_estimator_reports_the_pooled_auc(tmp_path):
    model_dir = str(tmp_path / "m")
    calls = []

    def factory():
        calls.append(1)
        return BinaryClassificationMetrics()

    est = _identity_estimator(
        model_dir, eval_metrics=factory,
        metrics_fn=lambda out, labels: {"accuracy": -1.0, "batch_n":
                                        float(labels.numel())})
    result = est.evaluate(lambda: iter(_EVAL_BATCHES))
    per_batch = [_result(x, y)["auc"] for x, y in _EVAL_BATCHES]
    assert per_batch == [1.0, 1.0]
    assert result["auc"] == 5 / 6
    assert set(KEYS) <= set(result)
    assert result["examples"] == 5.0
    assert result["accuracy"] == 3 / 5      # eval_metrics wins the clash
    assert result["batch_n"] == 2.5         # metrics_fn: still a batch mean
    assert len(calls) == 1
    events = get_all_metrics(model_dir)
    written = dict(zip(events["name"], events["value"]))
    for k in KEYS:
        assert written[k] == result[k], k
    again = est.evaluate(lambda: iter(_EVAL_BATCHES[:1]))
    assert len(calls) == 2                  # a fresh accumulator per evaluate
    assert again["examples"] == 2.0 and again["auc"] == 1.0


def test_estimator_without_eval_metrics_is_unchanged(tmp_path):
    est = _identity_estimator(str(tmp_path / "m"))
    result = est.evaluate(lambda: iter(_EVAL_BATCHES))
    assert set(result) == {"loss", "global_step"}


# ---- Keras shim -------------------------------------------------------------

def _keras_model():
    torch.manual_seed(0)
    return KerasModel(nn.Linear(4, 1)).to("cpu")


def _keras_data(n=64):
    g = torch.Generator().manual_seed(8)
    x = torch.randn(n, 4, generator=g)
    y = (x.sum(dim=1) + torch.randn(n, generator=g) > 0).float()
    return x, y


def test_keras_evaluate_return_dict():
    model = _keras_model()
    model.compile(optimizer="sgd", loss="binary_crossentropy",
                  metrics=["AUC", "accuracy", "pr_auc"])
    x, y = _keras_data()
    out = model.evaluate(x, y, batch_size=16, return_dict=True)
    assert set(out) == {"loss", "auc", "accuracy", "pr_auc"}
    pooled = _result(model.predict(x), y)
    assert out["auc"] == pooled["auc"]
    assert out["accuracy"] == pooled["accuracy"]
    assert out["pr_auc"] == pooled["auc_precision_recall"]
    loss = model.evaluate(x, y, batch_size=16)
    assert isinstance(loss, float) and loss == out["loss"]


def test_keras_fit_logs_val_metrics():
    seen = []

    class Capture(Callback):
        def on_epoch_end(self, epoch, logs, model):
            seen.append(dict(logs))

    model = _keras_model()
    model.compile(optimizer="sgd", loss="binary_crossentropy",
                  metrics=["AUC"])
    x, y = _keras_data()
    model.fit(x, y, epochs=2, batch_size=16, validation_data=(x, y),
              callbacks=[Capture()], verbose=0)
    assert len(seen) == 2
    for logs in seen:
        assert set(logs) == {"loss", "val_loss", "val_auc"}
        assert 0.0 <= logs["val_auc"] <= 1.0


def test_keras_unknown_metric_is_accepted_with_a_warning(caplog):
    model = _keras_model()
    with caplog.at_level(logging.WARNING,
                         logger="tf_yarn_amd.estimator.keras"):
        model.compile(optimizer="sgd", loss="binary_crossentropy",
                      metrics=["auc", "top_k_categorical_accuracy"])
    warnings = [r for r in caplog.records if r.levelno == logging.WARNING]
    assert len(warnings) == 1
    assert "top_k_categorical_accuracy" in warnings[0].getMessage()
    x, y = _keras_data()
    assert set(model.evaluate(x, y, batch_size=16, return_dict=True)) == \
        {"loss", "auc"}


def test_keras_saved_model_keeps_its_metrics(tmp_path):
    model = _keras_model()
    model.compile(optimizer="sgd", loss="binary_crossentropy",
                  metrics=["auc"])
    model.save(str(tmp_path / "checkpoint-0"))
    assert load_model(str(tmp_path / "checkpoint-0")).metrics == ["auc"]
