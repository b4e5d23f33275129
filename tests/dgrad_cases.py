"""Shared operands and references for the dgrad_drelu / MLPHeadFn tests
(``test_dgrad_drelu_gpu.py`` on the GPU, ``test_dgrad_drelu_cpu.py`` for
the fallbacks).  Everything here runs on the CPU."""

import torch

import exact_ints

BF16 = torch.bfloat16

# the values y mixes: positives, both zeros, a negative and a NaN; only the
# positives pass ``y > 0``
Y_VALUES = torch.tensor([1.0, 2.0, 3.0, 0.0, -0.0, -1.0, float("nan")])


def mixed_y(m, n, gen):
    return Y_VALUES[torch.randint(0, len(Y_VALUES), (m, n), generator=gen)]


def dgrad_operands(m, k, n, seed, saturate=True):
    """``dz_next [m, k]``, ``w [k, n]`` in [-2, 2] and a mixed ``y``.  With
    ``saturate`` the first rows of ``dz_next`` are all 2 and the first 32
    columns of ``w`` are 1 or 2, so that corner's sums are near ``3 * k``
    (exactly ``4 * k`` in columns 24..31) and, from k = 128 on, need more
    than bf16's 8 bits."""
    exact_ints.assert_exact(2, 2, k)       # the contraction
    exact_ints.assert_exact(2, 2, k * m)   # a column sum of |dz| <= 4 k
    gen = torch.Generator().manual_seed(seed)
    a = exact_ints.ints((m, k), 2, gen)
    w = exact_ints.ints((k, n), 2, gen)
    y = mixed_y(m, n, gen)
    if saturate:
        a[:8] = 2
        w[:, :min(n, 24)] = torch.randint(1, 3, (k, min(n, 24)),
                                          generator=gen, dtype=torch.int16)
        w[:, 24:32] = 2
        y[:8, :32] = 1.0
    return a, w, y


def dgrad_reference(a, w, y):
    """float64 ``(dz, dbias)``: dz is rounded to bf16 once, the column sums
    are of the rounded values."""
    acc = a.double() @ w.double()
    dz = torch.where(y > 0, exact_ints.rne_bf16(acc).double(),
                     torch.zeros_like(acc))
    return acc, dz, dz.sum(0)


# ---- the tower: 48 -> 64 -> 32 -> 16 -> 1 at batch 256 ---------------------

TOWER_BATCH = 256
TOWER_WIDTHS = (48, 64, 32, 16)


def _sparse_ints(rows, cols, per_row, gen):
    """[-1, 1] integers with ``per_row`` nonzero candidates per row."""
    w = torch.zeros(rows, cols, dtype=torch.int16)
    for r in range(rows):
        idx = torch.randperm(cols, generator=gen)[:per_row]
        w[r, idx] = torch.randint(0, 2, (per_row,), generator=gen,
                                  dtype=torch.int16) * 2 - 1
    return w


def tower_operands(seed=48):
    """Integer leaves ``(x, w_head, b_head, weights, biases)`` and ``dl``.
    Layer 0 is dense in [-1, 1] on x in [-2, 2] (|z| <= 98); the layers
    above have 2 nonzeros per weight row, so every activation stays an
    integer <= 256 that bf16 holds, every gradient that flows down is a
    small integer, and the float64 reference needs no rounding anywhere
    but at the returned gradients."""
    gen = torch.Generator().manual_seed(seed)
    d = TOWER_WIDTHS
    x = exact_ints.ints((TOWER_BATCH, d[0]), 2, gen)
    weights = [exact_ints.ints((d[1], d[0]), 1, gen),
               _sparse_ints(d[2], d[1], 2, gen),
               _sparse_ints(d[3], d[2], 1, gen)]
    biases = [exact_ints.ints((h,), 2, gen) for h in d[1:]]
    w_head = exact_ints.ints((d[3],), 1, gen)
    b_head = exact_ints.ints((1,), 2, gen)
    dl = exact_ints.ints((TOWER_BATCH,), 2, gen)
    return x, w_head, b_head, weights, biases, dl


def tower_reference(x, w_head, b_head, weights, biases, dl):
    """float64 autograd: gradients in the order (x, w_head, b_head,
    *weights, *biases), and the forward output.  Asserts that every
    activation is a value bf16 holds exactly."""
    leaves = [t.double().requires_grad_()
              for t in (x, w_head, b_head, *weights, *biases)]
    n = len(weights)
    h = leaves[0]
    for w, b in zip(leaves[3:3 + n], leaves[3 + n:]):
        h = torch.relu(h @ w.t() + b)
        assert h.abs().max() <= exact_ints.BF16_INT_MAX
    out = h @ leaves[1] + leaves[2]
    assert torch.equal(exact_ints.rne_bf16(out.detach()).double(),
                       out.detach())
    out.backward(dl.double())
    return [t.grad for t in leaves], out.detach()


def run_tower(fn, x, w_head, b_head, weights, biases, dl, device):
    """``fn(x, weights, biases, w_head, b_head)`` on bf16 leaves; returns
    gradients in :func:`tower_reference`'s order and the output."""
    leaves = [t.to(BF16).to(device).requires_grad_()
              for t in (x, w_head, b_head, *weights, *biases)]
    n = len(weights)
    out = fn(leaves[0], leaves[3:3 + n], leaves[3 + n:], leaves[1],
             leaves[2])
    out.backward(dl.to(BF16).to(device))
    return [t.grad for t in leaves], out.detach()
