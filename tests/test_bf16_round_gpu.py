"""``f32_to_bf16`` / ``bf16_to_f32`` (``csrc/common.h``) on the GPU, bit for
bit, through ``ops.convert_scaled``; and NaN propagation into the bf16
outputs of the kernels that use the helper.

The pattern sets and the integer round-to-nearest-even come from
``tests/optim_refs.py``.  Non-NaN patterns must give the integer RNE
(fp32 denormals and the overflow of ``0x7f7fffff`` to Inf included); every
NaN must come out a NaN, which for this helper is ``0x7fc0``.
"""

import numpy as np
import pytest
import torch

import optim_refs as R
from tf_yarn_amd import ops

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")

CANARY = 7.0
NAN_BITS = (0x7fffffff, 0x7f800001, 0xffffffff)


def _check_narrowed(src_bits, out):
    """``out`` (bf16 tensor) is the right narrowing of ``src_bits``."""
    got = R.bits_of(out)
    nan = R.is_nan_bits(src_bits)
    assert np.array_equal(got[~nan], R.rne_bf16_bits(src_bits[~nan]))
    assert bool(torch.isnan(out.cpu()[torch.from_numpy(nan)]).all())
    assert (got[nan] == R.BF16_QNAN).all()


def _check_widened(src_bits, out):
    """``out`` (fp32 tensor) is ``src_bits << 16``; NaNs stay NaNs."""
    want = src_bits.astype(np.uint32) << np.uint32(16)
    nan = R.is_nan_bits(want)
    assert np.array_equal(R.bits_of(out)[~nan], want[~nan])
    assert bool(torch.isnan(out.cpu()[torch.from_numpy(nan)]).all())


def _buffer(n, off, dtype):
    buf = torch.full((n + 8,), CANARY, dtype=dtype, device="cuda")
    assert buf.data_ptr() % 16 == 0
    return buf, buf[off:off + n]


def _untouched(buf, off, n):
    return bool((buf[:off] == CANARY).all()) and \
        bool((buf[off + n:] == CANARY).all())


@requires_gpu
def test_f32_to_bf16_every_pattern():
    bits = R.f32_patterns()
    assert int(R.is_nan_bits(bits).sum()) == 1534
    src = R.f32_from_bits(bits).cuda()
    dst = torch.empty(bits.size, dtype=torch.bfloat16, device="cuda")
    ops.convert_scaled(src, dst, 1.0)
    _check_narrowed(bits, dst)


@requires_gpu
def test_bf16_to_f32_every_pattern():
    bits = R.bf16_patterns()
    src = R.bf16_from_bits(bits).cuda()
    dst = torch.empty(bits.size, dtype=torch.float32, device="cuda")
    ops.convert_scaled(src, dst, 1.0)
    _check_widened(bits, dst)


@requires_gpu
@pytest.mark.parametrize("src_off,dst_off", [(0, 0), (0, 1), (1, 0), (1, 1),
                                             (2, 3), (3, 2)])
def test_f32_to_bf16_odd_length_and_placement(src_off, dst_off):
    """``n % 4 == 3`` and views at odd element offsets: the scalar tail,
    and the scalar loop for everything where a pointer is not aligned."""
    bits = R.f32_patterns()[:-1]
    n = bits.size
    assert n % 4 == 3
    sbuf, src = _buffer(n, src_off, torch.float32)
    src.copy_(R.f32_from_bits(bits))
    dbuf, dst = _buffer(n, dst_off, torch.bfloat16)
    ops.convert_scaled(src, dst, 1.0)
    _check_narrowed(bits, dst)
    assert _untouched(dbuf, dst_off, n)
    assert np.array_equal(R.bits_of(src), bits)  # the source is only read


@requires_gpu
@pytest.mark.parametrize("src_off,dst_off", [(0, 0), (0, 1), (1, 0), (1, 1),
                                             (2, 3), (3, 2)])
def test_bf16_to_f32_odd_length_and_placement(src_off, dst_off):
    bits = R.bf16_patterns()[:-1]
    n = bits.size
    assert n % 4 == 3
    sbuf, src = _buffer(n, src_off, torch.bfloat16)
    src.copy_(R.bf16_from_bits(bits))
    dbuf, dst = _buffer(n, dst_off, torch.float32)
    ops.convert_scaled(src, dst, 1.0)
    _check_widened(bits, dst)
    assert _untouched(dbuf, dst_off, n)
    assert np.array_equal(R.bits_of(src), bits)


# ---- NaN propagation at the op level -----------------------------------------

N = 11  # two quads and a 3-element tail
NAN_AT = (1, 2, 3, 8, 9, 10)  # a vector position and a tail position each


def _nan_grad():
    """A gradient of ones with the three NaN patterns, built from their
    bits, in the first quad and in the tail."""
    bits = R.bits_of(torch.ones(N)).copy()
    bits[list(NAN_AT)] = np.array(NAN_BITS + NAN_BITS, dtype=np.uint32)
    g = R.f32_from_bits(bits).cuda()
    assert np.array_equal(R.bits_of(g), bits)  # the payloads reach the GPU
    return g


def _check_copy_follows_master(master, copy):
    nan = torch.isnan(master)
    assert nan.cpu().nonzero().flatten().tolist() == list(NAN_AT)
    assert torch.equal(torch.isnan(copy), nan)
    assert torch.equal(copy.cpu().view(torch.int16),
                       R.rne_bf16_of(master.cpu()).view(torch.int16))


@requires_gpu
def test_fused_sgd_nan_reaches_the_bf16_copy():
    p = torch.linspace(-1, 1, N).cuda()
    copy = torch.zeros(N, dtype=torch.bfloat16, device="cuda")
    ops.fused_sgd(p, _nan_grad(), None, copy, lr=0.1)
    _check_copy_follows_master(p, copy)


@requires_gpu
def test_fused_sgd_mt_nan_reaches_the_bf16_copy():
    ps = [torch.linspace(-1, 1, N).cuda() for _ in range(2)]
    copies = [torch.zeros(N, dtype=torch.bfloat16, device="cuda")
              for _ in range(2)]
    ops.fused_sgd_mt(ps, [_nan_grad(), _nan_grad()], None, copies, lr=0.1)
    for p, copy in zip(ps, copies):
        _check_copy_follows_master(p, copy)


@requires_gpu
def test_fused_adam_nan_reaches_the_bf16_copy():
    p = torch.linspace(-1, 1, N).cuda()
    m = torch.zeros(N, device="cuda")
    v = torch.zeros(N, device="cuda")
    copy = torch.zeros(N, dtype=torch.bfloat16, device="cuda")
    ops.fused_adam(p, _nan_grad(), m, v, copy, lr=0.01, step=1)
    _check_copy_follows_master(p, copy)


@requires_gpu
@pytest.mark.parametrize("dim", [16, 7])  # the quad and the scalar gather
def test_emb_fwd_bf16_keeps_nans(dim):
    rows = 5
    bits = R.bits_of(torch.arange(rows * dim, dtype=torch.float32)
                     .reshape(rows, dim)).copy()
    bits[2, 1:4] = np.array(NAN_BITS, dtype=np.uint32)
    table = R.f32_from_bits(bits.reshape(-1)).reshape(rows, dim).cuda()
    ids = torch.tensor([2, 0, 4, 2, 1], device="cuda")
    out = ops.emb_fwd(table, ids, out_bf16=True)
    want = R.rne_bf16_of(table.cpu().index_select(0, ids.cpu()))
    assert torch.equal(out.cpu().view(torch.int16), want.view(torch.int16))
    nan = torch.isnan(out.cpu())
    assert nan[0, 1:4].all() and nan[3, 1:4].all() and int(nan.sum()) == 6
