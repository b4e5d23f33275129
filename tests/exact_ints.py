"""Integer-valued operands for exact-arithmetic kernel tests.

bf16 holds every integer of magnitude <= 256 exactly, the product of two
such values is exact in fp32, and an fp32 sum of integers is exact in ANY
order while every partial sum stays below 2**24.  A correct kernel fed such
operands therefore reproduces the float64 reference bit for bit, whatever
its tiling, split-K order or MFMA accumulation order, and the tests compare
with ``torch.equal``: no tolerance to pick.

Everything here runs on the CPU; ``tests/test_exact_ints.py`` covers it.
"""

import torch

EXACT_LIMIT = 2 ** 24   # fp32 holds every integer below this exactly
BF16_INT_MAX = 256      # bf16 holds every integer up to this exactly


def assert_exact(amax_a, amax_b, k, extra=0):
    """Refuse a case whose worst-case partial sum ``amax_a * amax_b * k +
    extra`` (``extra``: a bias or the like added to the sum) could reach
    2**24, or whose operands bf16 could not hold."""
    assert 0 <= amax_a <= BF16_INT_MAX and 0 <= amax_b <= BF16_INT_MAX, \
        f"operand magnitudes {amax_a}, {amax_b} are not exact in bf16"
    worst = amax_a * amax_b * k + extra
    assert worst < EXACT_LIMIT, (
        f"worst-case partial sum {amax_a}*{amax_b}*{k}+{extra} = {worst} "
        f"reaches 2**24: the fp32 result would depend on summation order")


def ints(shape, amax, gen):
    """Uniform integers in [-amax, amax] as an int16 CPU tensor; cast with
    ``.double()`` for the reference and ``.to(dtype)`` for the kernel."""
    assert 0 <= amax <= BF16_INT_MAX
    return torch.randint(-amax, amax + 1, tuple(shape), generator=gen,
                         dtype=torch.int16)


def operands(shape_a, shape_b, k, *, amax_a=2, amax_b=2, extra=0, seed=0):
    """Two integer operands of a length-``k`` contraction, after checking
    that the contraction stays in the exact regime."""
    assert_exact(amax_a, amax_b, k, extra)
    gen = torch.Generator().manual_seed(seed)
    return ints(shape_a, amax_a, gen), ints(shape_b, amax_b, gen)


def rne_bf16(ref64):
    """What a kernel with a bf16 output must store for an exact fp32
    result: ``f32_to_bf16`` (csrc/common.h) and torch both round to
    nearest even."""
    return ref64.float().to(torch.bfloat16)


def bf16_half_ulp(ref64):
    """Half a bf16 ulp (8 significant bits) at each reference value: the
    error of ONE correct rounding of that value to bf16.  0 at 0."""
    _, exponent = torch.frexp(ref64)  # |ref| = m * 2**exponent, m in [.5, 1)
    tol = torch.ldexp(torch.ones_like(ref64), exponent - 9)
    return torch.where(ref64 == 0, torch.zeros_like(ref64), tol)
