"""float64 reference of ``ops.cross_layer`` straight from its definition
(docs/Kernels.md, "Cross layer"), for the CPU and the GPU tests."""

import torch

import exact_ints

NAMES = ("y", "v", "dx0", "dx", "dW", "dbias")


def ref64(x0, x, w, bias, g, v=None):
    """``(y, v, dx0, dx, dW, dbias)`` in float64; operands of any dtype, on
    the CPU.  The backward reads the ROUNDED ``dz`` and ``v`` the kernels
    read: ``v`` is ``rne_bf16`` of this function's own unless given."""
    x0, x, w, bias, g = (t.double() for t in (x0, x, w, bias, g))
    v32 = x @ w.t() + bias
    y = x0 * v32 + x
    v = exact_ints.rne_bf16(v32).double() if v is None else v.double()
    dz = exact_ints.rne_bf16(g * x0).double()
    return y, v32, g * v, dz @ w + g, dz.t() @ x, dz.sum(0)


def int_operands(b, d, seed=0, amax=2):
    """Integer ``(x0, x, w, bias, g)`` in [-amax, amax] as int16.  Every
    fp32 intermediate of the forward and the backward stays an integer
    below 2**24, exact in any order (the checks below; ``dz = g * x0`` is
    at most 256 and never rounds), so a correct kernel gives
    ``rne_bf16(ref64)`` bit for bit.  With ``amax = 16`` most results need a
    real rounding to bf16, exact ties among them."""
    assert amax <= 16 and d <= 528 and b <= 300
    assert 16 * 16 * 528 * 16 + 16 < exact_ints.EXACT_LIMIT  # the worst case
    exact_ints.assert_exact(amax, amax, d, extra=amax)         # v32
    # y = x0 * v32 + x as one exact fp32 value
    assert amax * (amax * amax * d + amax) + amax < exact_ints.EXACT_LIMIT
    exact_ints.assert_exact(amax * amax, amax, d, extra=amax)  # dx
    exact_ints.assert_exact(amax * amax, amax, b)              # dW
    exact_ints.assert_exact(amax * amax, 1, b)                 # dbias
    gen = torch.Generator().manual_seed(seed)
    return tuple(exact_ints.ints(s, amax, gen)
                 for s in ((b, d), (b, d), (d, d), (d,), (b, d)))
