"""Float64 statement of the lazy (sparse) Adam rule of the embedding tables.

One definition everywhere: ``torch.optim.SparseAdam`` on a coalesced
gradient (TF ``LazyAdam``).  For each unique id ``u`` of the update, with
``G = scale * (sum of its gradient rows)``, per element::

    m' = m + (1 - beta1) * (G - m)
    v' = v + (1 - beta2) * (G*G - v)
    w' = w - step_size * m' / (sqrt(v') + eps)
    step_size = lr * sqrt(1 - beta2^t) / (1 - beta1^t)

``t`` counts the updates applied to the table, this one included.  Rows not
in the update are neither read nor written; a touched row whose gradients
sum to 0 still decays ``m`` and ``v`` and moves ``w``.  ``eps`` sits outside
the root and is not divided by the bias correction.

``lazy_adam_step64`` is written straight from these lines, one Python
iteration per unique id, and shares no code with ``tf_yarn_amd.ops``;
``test_sparse_lazy_adam.py`` checks it against ``torch.optim.SparseAdam``
in float64 before anything is checked against it."""

import math

import torch


def exact_grads(gen, shape, dtype=torch.float32):
    """Integers / 8: exact in bf16 and fp32, and so is every partial sum,
    in any order (the recipe of ``test_sparse_ftrl_gpu._exact_grads``)."""
    return (torch.randint(-32, 33, shape, generator=gen).float() / 8).to(dtype)


def lazy_adam_step64(w, m, v, ids, rows, *, lr, step, beta1=0.9,
                     beta2=0.999, eps=1e-8, scale=1.0):
    """One update, in place on the float64 tensors ``w``, ``m``, ``v``
    (``[rows, dim]``); ``rows`` are the gradient rows of ``ids``."""
    assert w.dtype == m.dtype == v.dtype == torch.float64
    flat = ids.reshape(-1)
    rows = rows.double().reshape(flat.numel(), -1)
    step_size = lr * math.sqrt(1.0 - beta2 ** step) / (1.0 - beta1 ** step)
    for u in sorted(set(flat.tolist())):
        g = scale * rows[flat == u].sum(dim=0)
        m1 = m[u] + (1.0 - beta1) * (g - m[u])
        v1 = v[u] + (1.0 - beta2) * (g * g - v[u])
        w[u] = w[u] - step_size * m1 / (v1.sqrt() + eps)
        m[u], v[u] = m1, v1


def wide_rows(gw, fan):
    """The per-update gradient rows ``[n, 1]`` of a wide table from the
    per-example ``gw`` (update i belongs to example ``i // fan``)."""
    return gw.float().reshape(-1, 1).expand(-1, fan).reshape(-1, 1)
