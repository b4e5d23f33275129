"""float64 reference of ``ops.dot_interaction`` straight from its
definition, for the CPU and the GPU tests."""

import torch

import exact_ints
from tf_yarn_amd import ops


def ref64(dense_vec, emb, grad_out=None):
    """``out [B, W]`` in float64, and with ``grad_out`` also
    ``(d_dense_vec, d_emb)``; operands of any dtype, on the CPU."""
    b, d = dense_vec.shape
    n = emb.shape[1] // d + 1
    t = torch.cat([dense_vec, emb], dim=1).double().reshape(b, n, d)
    i, j = torch.tril_indices(n, n, offset=-1)
    out = torch.zeros(b, ops.dot_interaction_width(n - 1, d),
                      dtype=torch.float64)
    out[:, :d] = t[:, 0]
    out[:, d:d + i.numel()] = torch.einsum("bpk,bpk->bp", t[:, i], t[:, j])
    if grad_out is None:
        return out
    g = grad_out.double()
    s = torch.zeros(b, n, n, dtype=torch.float64)
    s[:, i, j] = s[:, j, i] = g[:, d:d + i.numel()]
    dt = torch.einsum("bik,bkc->bic", s, t)
    dt[:, 0] += g[:, :d]
    return out, dt[:, 0], dt[:, 1:].reshape(b, -1)


def int_operands(b, n, d, seed=0, amax=2):
    """Integer ``(dense_vec, emb, grad_out)`` in [-amax, amax] as int16.
    With ``amax = 2`` every value of all three results is an integer below
    256, which bf16 holds; ``amax = 16`` keeps fp32 exact in any order (the
    checks below) and makes a quarter to a half of the results inexact in
    bf16, exact ties among them.  At ``amax = 2``, ``d = 128`` rows 0 and 1
    of every example are all 2 but for a 1 in column 5: their dot product
    is 4 * 127 + 1 = 509, an odd integer that bf16 (ulp 2 there) must round
    to the even 508."""
    exact_ints.assert_exact(amax, amax, d)
    exact_ints.assert_exact(amax, amax, 32, extra=amax)
    gen = torch.Generator().manual_seed(seed)
    dense_vec = exact_ints.ints((b, d), amax, gen)
    emb = exact_ints.ints((b, (n - 1) * d), amax, gen)
    g = exact_ints.ints((b, ops.dot_interaction_width(n - 1, d)), amax, gen)
    if amax == 2 and d == 128:
        dense_vec[:] = 2
        emb[:, :d] = 2
        dense_vec[:, 5] = emb[:, 5] = 1
    return dense_vec, emb, g


def pitched(t, pitch, fill=float("nan")):
    """``t [B, C]`` as the first ``C`` columns of a new ``[B, pitch]``
    buffer on ``t``'s device whose other columns hold ``fill``: a view with
    row stride ``pitch``."""
    b, c = t.shape
    wide = torch.full((b, pitch), fill, dtype=t.dtype, device=t.device)
    wide[:, :c] = t
    view = wide[:, :c]
    assert view.stride() == (pitch, 1) or b == 1
    return view


def same_bits(a, b):
    """``torch.equal`` that takes NaN for equal to NaN: same shape, same
    NaN mask, and the same values (Inf signs included) elsewhere."""
    return (a.shape == b.shape and torch.equal(a.isnan(), b.isnan())
            and torch.equal(a[~a.isnan()], b[~b.isnan()]))


def poison_emb(emb, d):
    """``emb`` with example 1 poisoned: +Inf in row 3 of its ``T``, NaN in
    row 7 (``N >= 9``)."""
    emb = emb.clone()
    emb[1, 2 * d + 5] = float("inf")
    emb[1, 6 * d + 2] = float("nan")
    return emb


def poison_grad(g, d):
    """``grad_out`` with example 1 poisoned: -Inf in a pass-through column,
    +Inf and NaN in two pair columns (``N >= 9``)."""
    g = g.clone()
    g[1, 3] = -float("inf")
    g[1, d + 3] = float("inf")     # pair (3, 0): reaches d_dense_vec
    g[1, d + 30] = float("nan")    # pair (8, 2)
    return g
