"""float64 reference of ``ops.cross_layer_lowrank`` straight from its
definition (docs/Kernels.md, "Low-rank cross layer")."""

import torch

import exact_ints

NAMES = ("y", "t", "v", "dx0", "dt", "dx", "dU", "dV", "dbias")


def ref64(x0, x, vw, uw, bias, g, t=None, v=None, dt=None):
    """``NAMES`` in float64 (``t``, ``v``, ``dt`` before their rounding).
    What reads a rounded intermediate (``t``, ``v``, ``dt``, ``dz``) reads
    ``rne_bf16`` of this function's own, or the one given."""
    x0, x, vw, uw, bias, g = (a.double() for a in (x0, x, vw, uw, bias, g))
    t32 = x @ vw.t()
    t = exact_ints.rne_bf16(t32).double() if t is None else t.double()
    v32 = t @ uw.t() + bias
    v = exact_ints.rne_bf16(v32).double() if v is None else v.double()
    dz = exact_ints.rne_bf16(g * x0).double()
    dt32 = dz @ uw
    dt = exact_ints.rne_bf16(dt32).double() if dt is None else dt.double()
    return (x0 * v32 + x, t32, v32, g * v, dt32, dt @ vw + g, dz.t() @ t,
            dt.t() @ x, dz.sum(0))


def int_operands(b, d, r, seed=0, amax=2, wmax=2):
    """Integer ``(x0, x, v_weight, u_weight, bias, g)`` as int16: data in
    [-amax, amax], both weights in [-wmax, wmax].  Asserts, by running the
    definition on the absolute values, that every fp32 intermediate stays
    below 2**24 (``dz = g * x0`` is at most 256 and never rounds): exact in
    any order, so a correct kernel gives ``rne_bf16(ref64)`` bit for bit."""
    assert amax <= 16 and wmax <= exact_ints.BF16_INT_MAX
    gen = torch.Generator().manual_seed(seed)
    x0, x, vw, uw, bias, g = (
        exact_ints.ints(s, m, gen)
        for s, m in (((b, d), amax), ((b, d), amax), ((r, d), wmax),
                     ((d, r), wmax), ((d,), amax), ((b, d), amax)))
    for name, mag in zip(NAMES, ref64(*(a.abs() for a in
                                        (x0, x, vw, uw, bias, g)))):
        assert mag.max() < exact_ints.EXACT_LIMIT, (name, mag.max())
    return x0, x, vw, uw, bias, g
