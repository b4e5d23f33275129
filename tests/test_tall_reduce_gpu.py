"""Tests of ``reduce_splitk``'s tall-slab kernel: ``out[c] = sum_s
part[s][c]`` for the deep stacks of narrow fp32 partial rows that the
dbias and ``col_reduce_dot`` kernels write (``S > 64`` or ``nm < 1024``),
which went to ``torch.sum`` before.

Integer operands (exact_ints.py) make every fp32 sum exact in any order,
so those cases are ``torch.equal`` against float64.  Powers of two and a
one-hot slab show a dropped, doubled or misplaced row.  Random floats get
the bound of an fp32 sum in ANY order, and two calls must agree to the
bit.  Each shape is there for one branch of the launch arithmetic
(elementwise.hip: 256 row lanes per block, 16 rows per lane and trip, a
block-to-quad map that depends on the block count modulo 8).
"""

import functools

import pytest
import torch

import exact_ints

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")

F32, BF16 = torch.float32, torch.bfloat16

# slab shape -> branch
EXACT_SHAPES = [
    (65, 1024),      # just past the S <= 64 of the split-K kernel
    (3, 512),        # narrow: nm < 1024, 253 idle row lanes
    (1, 4),          # one row, one quad, one block
    (255, 256),      # one row lane idle
    (256, 256),      # every row lane exactly one row
    (257, 256),      # row lane 0 takes a second row
    (8192, 256),     # the step's dbias slab: two full trips of 16 rows
    (4096 + 300, 16),  # 4 blocks (< 8 XCDs); a ragged second trip
    (300, 516),      # 129 quads: 129 % 8 == 1 uneven XCD shares
    (70, 4, 8),      # 3-D slab, the wgrad callers' layout
]


def _C():
    import tf_yarn_amd.ops._C as C
    return C


def _check_exact(out, ref64, out_bf16, shape):
    assert out.shape == tuple(shape[1:])
    if out_bf16:
        assert out.dtype == BF16
        assert torch.equal(out.cpu(), exact_ints.rne_bf16(ref64))
    else:
        assert out.dtype == F32
        assert torch.equal(out.cpu(), ref64.float())


@requires_gpu
@pytest.mark.parametrize("out_bf16", [False, True])
@pytest.mark.parametrize("shape", EXACT_SHAPES,
                         ids=["x".join(map(str, s)) for s in EXACT_SHAPES])
def test_integer_slabs_exact(shape, out_bf16):
    exact_ints.assert_exact(2, 1, shape[0])
    assert shape[0] <= 16384
    gen = torch.Generator().manual_seed(sum(shape))
    part = exact_ints.ints(shape, 2, gen)
    out = _C().reduce_splitk(part.to(F32).cuda(), out_bf16)
    _check_exact(out, part.double().sum(0), out_bf16, shape)


@requires_gpu
@pytest.mark.parametrize("out_bf16", [False, True])
@pytest.mark.parametrize("quad_lanes", [1, 4])
@pytest.mark.parametrize("shape", [(1, 4), (257, 256), (300, 516),
                                   (4096 + 300, 16)],
                         ids=["1x4", "257x256", "300x516", "4396x16"])
def test_both_maps_exact(shape, quad_lanes, out_bf16):
    """The kernel as bound for measurement, with 1 and with 4 quad lanes
    per block; 1 and 129 quads leave lanes of the 4-lane map without a
    column."""
    gen = torch.Generator().manual_seed(sum(shape) + quad_lanes)
    part = exact_ints.ints(shape, 2, gen)
    out = _C().reduce_tall(part.to(F32).cuda(), out_bf16, quad_lanes)
    _check_exact(out, part.double().sum(0), out_bf16, shape)


@requires_gpu
@pytest.mark.parametrize("out_bf16", [False, True])
def test_powers_of_two(out_bf16):
    """part[s][c] = 2^s over S = 20 rows: the sum is 2^20 - 1, all 20
    bits set, only if every row is added exactly once."""
    S, nm = 20, 256
    part = torch.pow(2.0, torch.arange(S, dtype=torch.float64)) \
        .unsqueeze(1).expand(S, nm).contiguous()
    out = _C().reduce_splitk(part.to(F32).cuda(), out_bf16)
    want = torch.full((nm,), float(2 ** 20 - 1), dtype=torch.float64)
    _check_exact(out, want, out_bf16, (S, nm))


@requires_gpu
@pytest.mark.parametrize("out_bf16", [False, True])
@pytest.mark.parametrize("S,nm", [(8192, 256), (1000, 516), (5, 16)])
def test_one_hot_names_its_column(S, nm, out_bf16):
    """part[(37*c) % S][c] = (c % 256) + 1, zero elsewhere."""
    c = torch.arange(nm)
    part = torch.zeros(S, nm, dtype=torch.float64)
    part[(37 * c) % S, c] = ((c % 256) + 1).double()
    out = _C().reduce_splitk(part.to(F32).cuda(), out_bf16)
    _check_exact(out, ((c % 256) + 1).double(), out_bf16, (S, nm))


@functools.lru_cache(maxsize=None)
def _random_slab():
    gen = torch.Generator().manual_seed(8192 + 256)
    part = torch.randn(8192, 256, generator=gen)
    return part, part.double().sum(0), part.double().abs().sum(0)


@requires_gpu
@pytest.mark.parametrize("out_bf16", [False, True])
def test_random_floats_bound_and_repeatable(out_bf16):
    part, ref, ref_abs = _random_slab()
    S = part.shape[0]
    dev = part.cuda()
    a = _C().reduce_splitk(dev, out_bf16)
    b = _C().reduce_splitk(dev.clone(), out_bf16)
    assert torch.equal(a, b)
    # an fp32 sum of S terms in any order: |err| <= S * 2^-24 * sum |x|
    bound = S * 2.0 ** -24 * ref_abs
    if out_bf16:
        bound = bound + exact_ints.bf16_half_ulp(ref)
    err = (a.double().cpu() - ref).abs()
    print("max err / bound:", (err / bound).max().item())
    assert (err <= bound).all()


@requires_gpu
@pytest.mark.parametrize("out_bf16", [False, True])
def test_wgrad_slab_keeps_the_split_k_kernel(out_bf16):
    """(28, 1024*432) is a wgrad slab (S <= 64, nm >= 1024): it stays on
    reduce_splitk_kernel, whose sum is a plain loop over ascending s."""
    gen = torch.Generator().manual_seed(28)
    part = torch.randn(28, 1024, 432, generator=gen).cuda()
    out = _C().reduce_splitk(part, out_bf16)
    acc = part[0].clone()
    for s in range(1, part.shape[0]):
        acc = acc + part[s]
    assert out.shape == (1024, 432)
    assert torch.equal(out, acc.to(BF16) if out_bf16 else acc)
