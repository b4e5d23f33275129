"""float64 reference of ``ops.field_attention`` from its definition
(docs/Kernels.md, "Field attention"), the operand builders of the exact
cases and the error bound of the random ones."""

import types

import torch

import exact_ints

NAMES = ("out", "dQ", "dK", "dV")
EPS = 2.0 ** -23


def _heads(t, n, h):
    """``[B*N, H*d] -> [B, H, N, d]`` in float64."""
    return t.double().reshape(-1, n, h, t.shape[1] // h).transpose(1, 2)


def _rows(t):
    """``[B, H, N, d] -> [B*N, H*d]``."""
    b, h, n, d = t.shape
    return t.transpose(1, 2).reshape(b * n, h * d)


def _rne(t):
    return exact_ints.rne_bf16(t).double()


def ref64(qkv, g, n, h, scale):
    """The definition in float64 with ``Pb`` and ``dSb`` rounded to bf16;
    ``.results`` is ``(out, dQ, dK, dV)`` as ``[B*N, H*d]``, the other
    fields are the ``[B, H, N, *]`` intermediates."""
    r = types.SimpleNamespace(scale=scale)
    hd = qkv.shape[1] // 3
    r.q, r.k, r.v = (_heads(qkv[:, i * hd:(i + 1) * hd], n, h)
                     for i in range(3))
    r.g = _heads(g, n, h)
    s = scale * r.q @ r.k.transpose(-1, -2)
    r.p = torch.exp(s - s.amax(-1, keepdim=True))
    r.pb = _rne(r.p / r.p.sum(-1, keepdim=True))
    r.dp = r.g @ r.v.transpose(-1, -2)
    r.delta = (r.pb * r.dp).sum(-1, keepdim=True)
    r.ds = scale * r.pb * (r.dp - r.delta)
    r.dsb = _rne(r.ds)
    r.results = tuple(_rows(t) for t in (
        r.pb @ r.v, r.dsb @ r.k, r.dsb.transpose(-1, -2) @ r.q,
        r.pb.transpose(-1, -2) @ r.g))
    return r


def _pack(q, k, v):
    return torch.cat([_rows(t) for t in (q, k, v)], dim=1)


def _ints(b, n, h, d, gen):
    return exact_ints.ints((b, h, n, d), 2, gen).double()


def selective(b, n, h, d, seed=0):
    """``(qkv, g, scale, ref)`` with exactly one-hot attention: ``K[j] =
    4 w_j``, ``Q[i] = 8 w_sigma(i)``, ``w`` the rows of a Sylvester-Hadamard
    matrix and their negatives, ``sigma`` seeded and not injective.  The
    matching score is 128 and every other ``exp`` underflows in fp32."""
    gen = torch.Generator().manual_seed(seed)
    w = torch.ones(1, 1, dtype=torch.float64)
    while w.shape[0] < d:
        w = torch.cat([torch.cat([w, w], 1), torch.cat([w, -w], 1)], 0)
    w = torch.cat([w, -w], 0)
    sigma = torch.randint(0, n, (b, h, n), generator=gen)
    q, k = 8 * w[sigma], (4 * w[:n]).expand(b, h, n, d)
    v, g = _ints(b, n, h, d, gen), _ints(b, n, h, d, gen)
    scale = 4.0 / d
    qkv = _pack(q, k, v)
    r = ref64(qkv, _rows(g), n, h, scale)
    hot = torch.nn.functional.one_hot(sigma, n).bool()
    assert (r.p[hot] == 1).all() and (r.p[~hot] < 2.0 ** -150).all()
    assert torch.equal(r.pb, hot.double()) and not r.dsb.any()
    return qkv, _rows(g), scale, r


def uniform(b, n, h, d, zero, seed=0):
    """``(qkv, g, scale, ref)`` with ``Pb = 1/N`` exactly: ``zero`` = "q"
    (``Q = 0``: ``dQ`` is exercised, ``dK = 0``) or "k".  ``dS`` is a
    multiple of ``scale / N^2`` that fp32 holds, so ``dSb`` is a
    deterministic rounding and the products behind it sum exactly in any
    order: the checks below."""
    assert n & (n - 1) == 0
    gen = torch.Generator().manual_seed(seed)
    q, k, v, g = (_ints(b, n, h, d, gen) for _ in range(4))
    # small N and d seldom give a dS of more than bf16's 8 bits: plant
    # dP[0][0] = 4 d - 2 and an odd sum of the other dP[0][j]
    v[:, :, 0] = g[:, :, 0] = 2
    g[:, :, 0, 0] = 1
    v[:, :, 1:, 0] = 0
    v[:, :, 1, 0] = 1
    if zero == "q":
        q = torch.zeros_like(q)
    else:
        k = torch.zeros_like(k)
    scale = 0.25
    qkv = _pack(q, k, v)
    r = ref64(qkv, _rows(g), n, h, scale)
    assert torch.equal(r.pb, torch.full_like(r.pb, 1.0 / n))
    unit = scale / n ** 2
    for t in (r.ds, r.dsb):     # granularity; fp32 holds each value
        assert torch.equal(t / unit, (t / unit).round())
    assert (r.ds.abs() / unit).max() < exact_ints.EXACT_LIMIT
    assert (r.dsb != r.ds).any(), "no dSb needed rounding"
    other = (r.k if zero == "q" else r.q).abs()
    worst = (r.dsb.abs().transpose(-1, -2) if zero == "k"
             else r.dsb.abs()) @ other
    assert worst.max() / unit < exact_ints.EXACT_LIMIT
    # out, dV and delta: sums of at most N integers times 1/N
    exact_ints.assert_exact(2, 1, n)
    exact_ints.assert_exact(4 * d, 1, n)
    return qkv, _rows(g), scale, r


def _ulp(t):
    return 2 * exact_ints.bf16_half_ulp(t)


def bounds(r, n, d):
    """Error bounds of ``(out, dQ, dK, dV)`` for an implementation of the
    definition with fp32 sums, term by term:

    * half a bf16 ulp for the final rounding of each result;
    * ``(K + 2) * 2^-23 * mag`` for an fp32 sum of ``K`` products whose
      absolute values sum to ``mag``;
    * ``eP``: the fp32 ``p / l`` is off by far less than half a bf16 ulp,
      so ``Pb`` is the reference's or its neighbour: one ulp of ``Pb``;
    * ``eDS``: the fp32 ``x = scale * Pb * (dP - delta)`` is off by ``ex``
      (``eP`` through the factor ``Pb``, the fp32 error of ``dP``, the
      error of ``delta``, which sums ``eP |dP|``, ``Pb eDP`` and its own
      fp32 sum, and three fp32 roundings of the product), and two values
      ``ex`` apart round to bf16 values at most ``ex`` plus one ulp apart."""
    t = lambda x: x.transpose(-1, -2)  # noqa: E731
    q, k, v, g, pb = (x.abs() for x in (r.q, r.k, r.v, r.g, r.pb))
    e_p = _ulp(pb)
    e_dp = (d + 2) * EPS * (g @ t(v))
    e_delta = ((e_p * r.dp.abs() + (pb + e_p) * e_dp).sum(-1, keepdim=True)
               + (n + 2) * EPS * (pb * r.dp.abs()).sum(-1, keepdim=True))
    ex = (r.scale * (e_p * (r.dp - r.delta).abs()
                     + (pb + e_p) * (e_dp + e_delta))
          + 3 * EPS * r.ds.abs())
    e_ds = ex + _ulp(r.ds.abs() + ex)
    ds = r.dsb.abs() + e_ds
    acc = (n + 2) * EPS
    inner = (e_p @ v + acc * (pb @ v),
             e_ds @ k + acc * (ds @ k),
             t(e_ds) @ q + acc * (t(ds) @ q),
             t(e_p) @ g + acc * (t(pb) @ g))
    return tuple(exact_ints.bf16_half_ulp(want) + _rows(e)
                 for want, e in zip(r.results, inner))


def normal(b, n, h, d, seed=1):
    """N(0, 1) bf16 ``(qkv, g)`` and the default scale."""
    gen = torch.Generator().manual_seed(seed)
    qkv = torch.randn(b * n, 3 * h * d, generator=gen).to(torch.bfloat16)
    g = torch.randn(b * n, h * d, generator=gen).to(torch.bfloat16)
    return qkv, g, d ** -0.5
