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


def int_operands(b, n, d, seed=0):
    """Integer ``(dense_vec, emb, grad_out)`` in [-2, 2] as int16.  At
    ``d = 128`` rows 0 and 1 of every example are all 2 but for a 1 in
    column 5: their dot product is 4 * 127 + 1 = 509, an odd integer that
    bf16 (ulp 2 there) must round to the even 508."""
    exact_ints.assert_exact(2, 2, d)
    exact_ints.assert_exact(2, 2, 32, extra=2)
    gen = torch.Generator().manual_seed(seed)
    dense_vec = exact_ints.ints((b, d), 2, gen)
    emb = exact_ints.ints((b, (n - 1) * d), 2, gen)
    g = exact_ints.ints((b, ops.dot_interaction_width(n - 1, d)), 2, gen)
    if d == 128:
        dense_vec[:] = 2
        emb[:, :d] = 2
        dense_vec[:, 5] = emb[:, 5] = 1
    return dense_vec, emb, g
