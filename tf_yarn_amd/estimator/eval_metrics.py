"""Streaming evaluation metrics of a binary classifier.

The TF canned binary classifiers write ``accuracy``, ``auc``,
``auc_precision_recall``, ``average_loss``, ``label/mean``,
``prediction/mean``, ``precision`` and ``recall`` into their eval event
files.  :class:`BinaryClassificationMetrics` produces the same keys over a
whole evaluation: each batch of logits and labels is folded into a small
device state by one HIP kernel (:func:`tf_yarn_amd.ops.binary_eval_update`,
no host sync), and :meth:`~BinaryClassificationMetrics.result` derives every
metric from one copy of that state.  Ranking metrics are therefore pooled
over all examples, never averaged over batches.

Scores are bucketed: 4096 buckets of width 1/128 in logit space over
``[-16, 16)``, the ends clamping.  AUC is invariant under the monotone
sigmoid, so bucketing logits loses nothing against bucketing
probabilities; logits closer than 1/128 may share a bucket and then count
as tied.  Sample weights are not supported.
"""

from __future__ import annotations

import math
from typing import Dict, Optional

import torch

from tf_yarn_amd import ops

KEYS = ("accuracy", "auc", "auc_precision_recall", "average_loss",
        "label/mean", "prediction/mean", "precision", "recall", "examples",
        "nan_examples")


def _ratio(num: int, den: int) -> float:
    return num / den if den else 0.0


class BinaryClassificationMetrics:
    """Accumulator over ``update(outputs, labels)`` calls; ``outputs`` are
    logits (``[n]`` or ``[n, 1]``), ``labels`` 0/1 (``>= 0.5`` is positive).
    Examples whose logit or label is NaN are counted in ``nan_examples``
    and enter nothing else."""

    def __init__(self, device=None):
        self._device = device
        self._state: Optional[ops.BinaryEvalState] = None

    def _ensure_state(self, device) -> ops.BinaryEvalState:
        if self._state is None:
            self._state = ops.BinaryEvalState(
                self._device if self._device is not None else device)
        return self._state

    def update(self, outputs: torch.Tensor, labels: torch.Tensor) -> None:
        if outputs.dim() > 1 and outputs.shape[-1] == 1:
            outputs = outputs.squeeze(-1)
        state = self._ensure_state(outputs.device)
        dev = state.hist.device
        ops.binary_eval_update(outputs.detach().to(dev),
                               torch.as_tensor(labels).to(dev), state)

    def reset(self) -> None:
        if self._state is not None:
            self._state.zero_()

    def merge(self, other: "BinaryClassificationMetrics") -> None:
        """Add ``other``'s state: the result is that of one accumulator fed
        both streams (exactly so for every key but the two float means)."""
        if other._state is None:
            return
        mine = self._ensure_state(other._state.hist.device)
        for a, b in zip(mine.tensors(), other._state.tensors()):
            a += b.to(a.device)

    def all_reduce(self, group=None) -> None:
        """SUM the state over the process group, after which every rank's
        ``result()`` is that of the pooled evaluation.  No-op without an
        initialised process group."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()):
            return
        for t in self._ensure_state("cpu").tensors():
            dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)

    def result(self) -> Dict[str, float]:
        """Every key of :data:`KEYS`.  Integer-derived metrics are computed
        in Python integers with one division at the end (the average
        precision: one division per bucket and an exactly rounded sum), so
        they do not depend on batch order, batch split or device.

        ``auc`` is the Mann-Whitney statistic of the bucketed scores with
        ties counted one half (``0.0`` when a class is absent, TF's
        convention).  ``auc_precision_recall`` is the average precision of
        the bucketed scores, a whole bucket as one tie: the step-sum
        estimator ``sum_k (recall_k - recall_{k+1}) * precision_k``, NOT
        TF's interpolated ``careful_interpolation`` summation."""
        if self._state is None:
            hist = [[0] * ops.EVAL_BUCKETS] * 2
            n_nan = tp = fp = 0
            loss_sum = sig_sum = 0.0
        else:
            hist = self._state.hist.cpu().tolist()
            _, n_nan, tp, fp = self._state.counts.cpu().tolist()
            loss_sum, sig_sum = self._state.sums.cpu().sum(dim=0).tolist()
        neg, pos = hist
        n_pos, n_neg = sum(pos), sum(neg)
        n = n_pos + n_neg

        pairs = 0  # 2 * (pos-above-neg pairs + half the ties)
        below = 0
        for k in range(ops.EVAL_BUCKETS):
            if pos[k]:
                pairs += pos[k] * (2 * below + neg[k])
            below += neg[k]

        ap_terms = []  # pos[k] * precision at threshold k, one rounding each
        tp_k = fp_k = 0
        for k in range(ops.EVAL_BUCKETS - 1, -1, -1):
            tp_k += pos[k]
            fp_k += neg[k]
            if pos[k]:
                ap_terms.append(pos[k] * tp_k / (tp_k + fp_k))

        return {
            "accuracy": _ratio(tp + n_neg - fp, n),
            "auc": _ratio(pairs, 2 * n_pos * n_neg),
            "auc_precision_recall":
                math.fsum(ap_terms) / n_pos if n_pos else 0.0,
            "average_loss": loss_sum / n if n else 0.0,
            "label/mean": _ratio(n_pos, n),
            "prediction/mean": sig_sum / n if n else 0.0,
            "precision": _ratio(tp, tp + fp),
            "recall": _ratio(tp, n_pos),
            "examples": float(n),
            "nan_examples": float(n_nan),
        }
