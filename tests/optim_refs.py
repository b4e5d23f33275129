"""Float64 references, bf16 rounding in integers and input generators for
the dense optimizer kernels (``csrc/fused_optimizers.hip``) and the bf16
conversions (``csrc/common.h``).

* ``sgd``, ``sgd_mt``, ``adam``, ``adagrad``, ``adadelta``, ``ftrl``: the six
  update rules in torch float64, written from the formulas in the kernels'
  comments and ``docs/Kernels.md``.  They take the arguments of the
  ``ops.fused_*`` calls, call no ``ops.*`` and return new tensors.
* ``rne_bf16_bits``: round-to-nearest-even fp32 -> bf16 on ``uint32`` bit
  patterns in integer arithmetic, for non-NaN patterns.
* ``f32_patterns`` / ``bf16_patterns``: the bit patterns the conversion
  tests walk.
* ``dyadic_sgd_case``: SGD operands for which every intermediate of the
  rule is exact in fp32, so a correct kernel equals the float64 reference
  bit for bit whichever multiply-adds the compiler contracts.
* ``warm_case``: random operands with states from two reference steps, and
  ``err_ulps``, the error measure the random-input tests bound.

Everything here runs on the CPU; ``tests/test_optim_refs.py`` covers it.
"""

import functools

import numpy as np
import torch

# ---- the six rules in float64 ---------------------------------------------


def sgd(p, g, m=None, *, lr, momentum=0.0, dampening=0.0, weight_decay=0.0,
        nesterov=False, first_step=False, grad_scale=1.0):
    """``(p', m')``; ``m=None`` is SGD without a momentum buffer."""
    g = g.double() * grad_scale + weight_decay * p
    if m is not None:
        m = g.clone() if first_step \
            else momentum * m + (1.0 - dampening) * g
        g = g + momentum * m if nesterov else m
    return p - lr * g, m


def sgd_mt(ps, gs, ms=None, **kw):
    """Multi-tensor SGD: the rule on every tensor of the lists."""
    out = [sgd(p, g, None if ms is None else ms[i], **kw)
           for i, (p, g) in enumerate(zip(ps, gs))]
    return [o[0] for o in out], (None if ms is None else [o[1] for o in out])


def adam(p, g, m, v, *, lr, beta1=0.9, beta2=0.999, eps=1e-8,
         weight_decay=0.0, adamw=False, step=1, grad_scale=1.0):
    """``(p', m', v')`` of Adam (L2 penalty in the gradient) or AdamW
    (decoupled decay of the weight)."""
    g = g.double() * grad_scale
    if adamw:
        p = p - lr * weight_decay * p
    else:
        g = g + weight_decay * p
    m = beta1 * m + (1.0 - beta1) * g
    v = beta2 * v + (1.0 - beta2) * g * g
    mhat = m / (1.0 - beta1 ** step)
    vhat = v / (1.0 - beta2 ** step)
    return p - lr * mhat / (vhat.sqrt() + eps), m, v


def adagrad(p, g, acc, *, lr, eps=1e-10, weight_decay=0.0, grad_scale=1.0):
    """``(p', acc')``."""
    g = g.double() * grad_scale + weight_decay * p
    acc = acc + g * g
    return p - lr * g / (acc.sqrt() + eps), acc


def adadelta(p, g, sq, acc_d, *, lr=1.0, rho=0.9, eps=1e-6,
             weight_decay=0.0, grad_scale=1.0):
    """``(p', square_avg', acc_delta')``."""
    g = g.double() * grad_scale + weight_decay * p
    sq = rho * sq + (1.0 - rho) * g * g
    dx = (acc_d + eps).sqrt() / (sq + eps).sqrt() * g
    acc_d = rho * acc_d + (1.0 - rho) * dx * dx
    return p - lr * dx, sq, acc_d


def ftrl(p, g, n, z, *, lr, l1=0.0, l2=0.0, grad_scale=1.0):
    """``(w', n', z')`` of dense FTRL-proximal (``learning_rate_power =
    -0.5``, no beta, no L2 shrinkage); ``w'`` is exactly 0 where
    ``|z'| <= l1``."""
    g = g.double() * grad_scale
    n_new = n + g * g
    r_new = n_new.sqrt()
    z_new = z + g - (r_new - n.sqrt()) / lr * p
    q = r_new / lr + 2.0 * l2
    w = torch.where(z_new.abs() > l1,
                    (torch.copysign(torch.full_like(z_new, l1), z_new)
                     - z_new) / q,
                    torch.zeros_like(z_new))
    return w, n_new, z_new


# One calling convention for the four stateful rules:
# RULES[name](p, g, *states, **kw) -> (p', *states').
RULES = {"adam": adam, "adagrad": adagrad, "adadelta": adadelta,
         "ftrl": ftrl}
STATE_NAMES = {"adam": ("exp_avg", "exp_avg_sq"), "adagrad": ("state_sum",),
               "adadelta": ("square_avg", "acc_delta"),
               "ftrl": ("accum", "linear")}

# ---- bf16 rounding on bit patterns ----------------------------------------

F32_LOW_HALVES = (0x0000, 0x0001, 0x7fff, 0x8000, 0x8001, 0xffff)
BF16_QNAN = 0x7fc0  # what f32_to_bf16 stores for every NaN


def is_nan_bits(bits):
    """NaN mask of fp32 bit patterns (``uint32`` array)."""
    return (bits & np.uint32(0x7fffffff)) > np.uint32(0x7f800000)


def rne_bf16_bits(bits):
    """fp32 bit patterns (``uint32``) -> the ``uint16`` bf16 patterns of
    round-to-nearest-even, in integer arithmetic.  NaN patterns are
    refused: adding the rounding increment can carry a NaN into Inf or
    zero."""
    bits = np.asarray(bits, dtype=np.uint32)
    assert not is_nan_bits(bits).any(), "rne_bf16_bits is for non-NaN bits"
    x = bits.astype(np.uint64)
    x = x + np.uint64(0x7fff) + ((x >> np.uint64(16)) & np.uint64(1))
    return ((x >> np.uint64(16)) & np.uint64(0xffff)).astype(np.uint16)


def f32_patterns():
    """All 65,536 high halves x the low halves ``F32_LOW_HALVES``: 393,216
    fp32 patterns.  The low halves are zero, the smallest non-zero, just
    below the tie, the tie, just above it and all ones; the high halves
    make the kept bit even and odd, and reach every exponent, both signs,
    the denormals, Inf and the NaNs."""
    hi = np.arange(1 << 16, dtype=np.uint32) << np.uint32(16)
    lo = np.array(F32_LOW_HALVES, dtype=np.uint32)
    return (hi[:, None] | lo[None, :]).reshape(-1)


def bf16_patterns():
    """All 65,536 bf16 patterns."""
    return np.arange(1 << 16, dtype=np.uint32).astype(np.uint16)


def f32_from_bits(bits):
    """A CPU fp32 tensor holding exactly these ``uint32`` patterns."""
    a = np.ascontiguousarray(np.asarray(bits, dtype=np.uint32))
    return torch.from_numpy(a.view(np.int32).copy()).view(torch.float32)


def bf16_from_bits(bits):
    """A CPU bf16 tensor holding exactly these ``uint16`` patterns."""
    a = np.ascontiguousarray(np.asarray(bits, dtype=np.uint16))
    return torch.from_numpy(a.view(np.int16).copy()).view(torch.bfloat16)


def bits_of(t):
    """The bit patterns of an fp32 (``uint32``) or bf16 (``uint16``)
    tensor, as a numpy array."""
    t = t.detach().cpu().contiguous()
    if t.dtype == torch.float32:
        return t.view(torch.int32).numpy().view(np.uint32)
    assert t.dtype == torch.bfloat16
    return t.view(torch.int16).numpy().view(np.uint16)


def rne_bf16_of(t32):
    """The bf16 tensor a correct ``f32_to_bf16`` stores for an fp32 tensor:
    integer RNE of its bits, ``BF16_QNAN`` where it is NaN."""
    bits = bits_of(t32)
    nan = is_nan_bits(bits)
    out = rne_bf16_bits(np.where(nan, np.uint32(0), bits))
    out[nan] = BF16_QNAN
    return bf16_from_bits(out).reshape(t32.shape)


# ---- dyadic SGD operands --------------------------------------------------

# Every value below is k * 2**-3 with |k| <= 64, and the scalars are small
# dyadic rationals.  With gs = g/2 (2**-4 units, |gs| <= 4):
#   gv = gs + p/8                      2**-6 units, |gv| <= 5
#   m' = m/2 + 3/4 * gv                2**-8 units, |m'| <= 7.75
#   gv + m'/2   (nesterov)             2**-9 units, |.|  <= 8.875
#   p' = p - (that)/4                  2**-11 units, |p'| <= 10.3
# so every product, sum and fused multiply-add of the rule has fewer than
# 2**15 units: exact in fp32 (24 bits) in any association, and p' (up to 15
# significant bits) still has to be ROUNDED to bf16 for the compute copy.
DYADIC_SGD_KW = dict(lr=0.25, momentum=0.5, dampening=0.25,
                     weight_decay=0.125, grad_scale=0.5)
DYADIC_AMAX = 64
DYADIC_UNIT = 2.0 ** -3


def dyadic(n, seed):
    """``n`` values ``k / 8``, ``k`` an integer in [-64, 64] that depends
    on the seed AND on the position, as a float64 tensor (exact in bf16)."""
    gen = torch.Generator().manual_seed(seed)
    r = torch.randint(0, 2 * DYADIC_AMAX + 1, (n,), generator=gen,
                      dtype=torch.int64)
    k = (r + 37 * torch.arange(n, dtype=torch.int64)) \
        % (2 * DYADIC_AMAX + 1) - DYADIC_AMAX
    return k.double() * DYADIC_UNIT


@functools.lru_cache(maxsize=None)
def dyadic_sgd_case(n, seed=0):
    """``(p, g, m)`` float64 dyadic operands of one SGD call.  Cached: the
    callers clone before they update in place."""
    return dyadic(n, 3 * seed), dyadic(n, 3 * seed + 1), \
        dyadic(n, 3 * seed + 2)


def assert_f32_exact(x64):
    """The float64 result survives a round trip through fp32."""
    assert torch.equal(x64.float().double(), x64), \
        "reference result is not exact in fp32"


# ---- random operands, warm states, the error measure -----------------------

# eps of Adam and Adagrad is 1e-3, not the default 1e-8 / 1e-10: next to
# sqrt(v) of order 1 a default eps is below half an fp32 ulp of the sum, and
# a kernel that put it inside the square root, or dropped it, would pass.
# At 1e-3 that moves the update by 5e-4 of itself, tens of ulps of p.
RULE_KW = {
    "adam": dict(lr=0.01, beta1=0.9, beta2=0.99, eps=1e-3,
                 weight_decay=0.01, step=3, grad_scale=0.5),
    "adagrad": dict(lr=0.05, eps=1e-3, weight_decay=0.01, grad_scale=0.5),
    "adadelta": dict(lr=1.0, rho=0.9, eps=1e-6, weight_decay=0.01,
                     grad_scale=0.5),
    "ftrl": dict(lr=0.05, l1=0.01, l2=0.001, grad_scale=0.5),
}
FTRL_INITIAL_ACCUM = 0.1
WARM_SEED = 0  # see ftrl_band_mask / test_optim_refs for the seed's condition


def _zero_states(rule, p):
    if rule == "ftrl":
        return (torch.full_like(p, FTRL_INITIAL_ACCUM), torch.zeros_like(p))
    return tuple(torch.zeros_like(p) for _ in STATE_NAMES[rule])


@functools.lru_cache(maxsize=None)
def warm_case(rule, n, adamw=False, seed=WARM_SEED):
    """fp32 operands of the THIRD step of ``rule``: ``p`` and the states
    after two float64 reference steps on N(0, 1) weights and gradients,
    rounded to fp32, and a fresh N(0, 1) fp32 gradient.  Returns
    ``(p, g, states, kw)``; cached, so callers clone."""
    gen = torch.Generator().manual_seed(
        1000 * seed + 17 * sorted(RULES).index(rule) + int(adamw))
    p = torch.randn(n, generator=gen, dtype=torch.float64)
    kw = dict(RULE_KW[rule])
    if rule == "adam":
        kw["adamw"] = adamw
    states = _zero_states(rule, p)
    for step in (1, 2):
        g = torch.randn(n, generator=gen, dtype=torch.float64)
        skw = dict(kw, step=step) if rule == "adam" else kw
        p, *states = RULES[rule](p, g, *states, **skw)
    g = torch.randn(n, generator=gen, dtype=torch.float64).float()
    return p.float(), g, tuple(s.float() for s in states), kw


def ulp32(x):
    """Spacing of fp32 at magnitude ``x`` (a Python float)."""
    return float(np.spacing(np.float32(abs(x))))


def err_ulps(x, ref64):
    """``E(x) = max_i |x_i - ref_i| / ulp32(max_j |ref_j|)``: the largest
    error of an fp32 tensor against the float64 reference, in fp32 ulps at
    the reference's largest magnitude."""
    ref64 = ref64.detach().cpu().double().reshape(-1)
    x = x.detach().cpu().double().reshape(-1)
    scale = ulp32(ref64.abs().max().item())
    return ((x - ref64).abs().max() / scale).item()


def ftrl_band_mask(p, g, n, z, *, lr, l1, l2=0.0, grad_scale=1.0):
    """Elements whose reference ``|z'|`` lies so close to ``l1`` that an
    fp32 evaluation may fall on the other side of the ``|z'| > l1`` test.
    ``z' = z + g - s * w`` with ``s = (sqrt(n') - sqrt(n)) / lr``: each of
    the three terms and the sum carries up to a rounding at its own
    magnitude, and the difference of the square roots is off by up to an
    ulp of ``sqrt(n')``, which ``w / lr`` multiplies.  The band is 4 times
    the sum of those two ulps."""
    p, g, n, z = (t.double() for t in (p, g, n, z))
    g = g * grad_scale
    r_new = (n + g * g).sqrt()
    s = (r_new - n.sqrt()) / lr
    z_new = z + g - s * p
    mag = torch.stack([z.abs(), g.abs(), (s * p).abs(),
                       torch.full_like(z, l1)]).max(dim=0).values
    as32 = lambda t: torch.from_numpy(  # noqa: E731
        np.spacing(t.float().numpy())).double()
    width = 4.0 * (as32(mag) + as32(r_new) * p.abs() / lr)
    return (z_new.abs() - l1).abs() <= width
