"""float64 reference of ``ops.cin_layer`` from its definition
(docs/Kernels.md, "CIN layer"), the operand builders of the exact cases and
the error bound of the random ones."""

import types

import torch

import exact_ints

NAMES = ("y", "dx", "dx0", "dW")
EPS = 2.0 ** -23
BF16 = torch.bfloat16

# (m, H_in, H_out, D)
SHAPES = [(2, 2, 16, 16), (5, 5, 16, 16), (27, 27, 32, 16),
          (27, 32, 48, 16), (32, 40, 64, 32), (31, 3, 16, 64),
          (8, 256, 256, 16)]
SMALL = SHAPES[:4]


def _rne(t):
    return exact_ints.rne_bf16(t).double()


def ref64(x0, x, w, g):
    """The definition in float64 with ``z`` rounded to bf16; ``.results`` is
    ``(y, dx, dx0, dW)`` in the op's layouts, the other fields are the
    operands as ``[B, m, D]``, ``[B, H_in, D]``, ``[B, H_out, D]`` and the
    intermediates."""
    r = types.SimpleNamespace()
    b, (h_out, h_in, m) = x0.shape[0], w.shape
    r.w = w.double()
    r.x0 = x0.double().reshape(b, m, -1)
    r.x = x.double().reshape(b, h_in, -1)
    r.g = g.double().reshape(b, h_out, -1)
    r.z_raw = r.x.unsqueeze(2) * r.x0.unsqueeze(1)
    r.z = _rne(r.z_raw)
    r.du = torch.einsum("bhc,hij->bijc", r.g, r.w)
    r.results = (
        torch.einsum("hij,bijc->bhc", r.w, r.z).reshape(b, -1),
        (r.du * r.x0.unsqueeze(1)).sum(2).reshape(b, -1),
        (r.du * r.x.unsqueeze(2)).sum(1).reshape(b, -1),
        torch.einsum("bhc,bijc->hij", r.g, r.z))
    return r


def _abs(r):
    """The same sums over absolute values: a bound on every partial sum."""
    a = types.SimpleNamespace(**{k: v.abs() for k, v in vars(r).items()
                                 if torch.is_tensor(v)})
    a.du = torch.einsum("bhc,hij->bijc", a.g, a.w)
    return a, (torch.einsum("hij,bijc->bhc", a.w, a.z),
               (a.du * a.x0.unsqueeze(1)).sum(2),
               (a.du * a.x.unsqueeze(2)).sum(1),
               torch.einsum("bhc,bijc->hij", a.g, a.z))


def ints(b, m, h_in, h_out, d, amax=2, first=False, seed=0):
    """``(x0, x, w, g, ref)`` of integers: ``w`` and ``g`` in [-2, 2], ``x0``
    and ``x`` in [-amax, amax] (``first``: ``x`` is ``x0``).  Every partial
    sum stays below 2**24, so fp32 sums are exact in any order.  With
    ``amax = 31`` many ``z`` need more than bf16's 8 bits: the builder
    checks that some were rounded, some of them on exact ties, and that a
    share of the results needs the final rounding."""
    gen = torch.Generator().manual_seed(seed)
    x0 = exact_ints.ints((b, m * d), amax, gen)
    x = x0 if first else exact_ints.ints((b, h_in * d), amax, gen)
    w = exact_ints.ints((h_out, h_in, m), 2, gen)
    g = exact_ints.ints((b, h_out * d), 2, gen)
    r = ref64(x0, x, w, g)
    a, sums = _abs(r)
    assert max(s.max() for s in sums) < exact_ints.EXACT_LIMIT
    assert (a.du * a.x0.unsqueeze(1)).max() < exact_ints.EXACT_LIMIT
    if amax > 16:
        rounded = r.z != r.z_raw
        # a tie: the product lies midway between two bf16 neighbours
        ulp = 2 * exact_ints.bf16_half_ulp(r.z_raw)
        ties = rounded & ((r.z_raw - r.z).abs() * 2 == ulp)
        assert rounded.float().mean() > 0.05 and ties.any()
        for want in r.results:
            assert (_rne(want) != want).float().mean() > 0.02
    return x0, x, w, g, r


def bounds(r):
    """Error bounds of ``(y, dx, dx0, dW)`` for an implementation of the
    definition with fp32 sums, term by term: half a bf16 ulp for the final
    rounding of each result, and ``(K + 2) * 2^-23 * mag`` for an fp32 sum
    of ``K`` products whose absolute values sum to ``mag``.  The product
    ``x * x0`` of two bf16 values is exact in fp32, so ``z`` is the
    reference's; ``dU`` (``K = H_out``) carries its own sum's error into
    the sums over ``j`` and ``i``."""
    b, (h_out, h_in, m) = r.x0.shape[0], r.w.shape
    d = r.x0.shape[2]
    a, (y, dx, dx0, dw) = _abs(r)
    e_du = (h_out + 2) * EPS * a.du
    inner = ((h_in * m + 2) * EPS * y,
             (e_du * a.x0.unsqueeze(1)).sum(2) + (m + 2) * EPS * dx,
             (e_du * a.x.unsqueeze(2)).sum(1) + (h_in + 2) * EPS * dx0,
             (b * d + 2) * EPS * dw)
    return tuple(exact_ints.bf16_half_ulp(want) + e.reshape(want.shape)
                 for want, e in zip(r.results, inner))


def normal(b, m, h_in, h_out, d, seed=1):
    """N(0, 1) bf16 ``(x0, x, w, g)``."""
    gen = torch.Generator().manual_seed(seed)
    return tuple(torch.randn(*s, generator=gen).to(BF16) for s in (
        (b, m * d), (b, h_in * d), (h_out, h_in, m), (b, h_out * d)))


def run(ops, x0, x, w, g, m, max_blocks=None, loss=None, device="cpu"):
    """``(y, dx, dx0, dW)`` of the public op through autograd, on the CPU;
    ``x is x0`` stays one leaf and ``dx``, ``dx0`` are then both its summed
    gradient; ``loss(y)`` replaces ``g``."""
    dev = lambda t: t.to(device=device, dtype=BF16)  # noqa: E731
    first = x is x0
    x0, w, g = dev(x0).detach().requires_grad_(), \
        dev(w).detach().requires_grad_(), dev(g)
    x = x0 if first else dev(x).detach().requires_grad_()
    y = ops.cin_layer(x0, x, w, m, max_blocks)
    leaves = (x0, w) if first else (x, x0, w)
    grads = torch.autograd.grad(y, leaves, g) if loss is None else \
        torch.autograd.grad(loss(y), leaves)
    if first:
        grads = (grads[0], grads[0], grads[1])
    return [t.detach().cpu() for t in (y, *grads)]


def expected(r, first=False):
    """``rne_bf16`` of the reference's results; with ``x is x0`` autograd
    hands back the bf16 sum of the two rounded gradients for both."""
    y, dx, dx0, dw = (exact_ints.rne_bf16(t) for t in r.results)
    if first:
        dx = dx0 = dx + dx0
    return y, dx, dx0, dw


def assert_exact(got, r, first=False):
    for name, a, want in zip(NAMES, got, expected(r, first)):
        assert a.dtype == BF16 and a.shape == want.shape, name
        assert torch.equal(a, want), name
