"""The LDS-DMA staging of the split-K weight-gradient kernels against
their register-staged control (``regstage=True``), bit for bit.

Both stagings feed the same MFMAs the same operand registers in the same
k order under the same split plan, so on any operands, N(0,1) bf16 here
so that every rounding matters, the two dW are ``torch.equal``.  The
exact-integer tests of test_dense_exact_gpu.py reach the default staging
through the unchanged entry points; this file pins the two against each
other where the sync structure differs:

* B = 64 (prologue and final compute only), 128 (each buffer once),
  192 (first buffer reuse), all with one slab;
* 320 with splitk=2 (slabs of 3 + 2 steps), 65*64 with auto split-K and
  splitk=4 (short last slab);
* M = 8, TILE+8, 432 (clamped source chunks, masked columns) and one or
  two N tiles; one case at the workload's depth.
"""

import pytest
import torch

import wgrad_image as wi
from tf_yarn_amd import ops

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")

BK = 64
KERNELS = (("wgrad_nt128", 128), ("wgrad_nt256", 256))


def _operands(B, N, M, seed):
    g = torch.Generator().manual_seed(seed)
    dy = torch.randn(B, N, generator=g).to(torch.bfloat16).cuda()
    x = torch.randn(B, M, generator=g).to(torch.bfloat16).cuda()
    return dy, x


def _cases():
    cases = []
    for name, tile in KERNELS:
        for B, splitk in ((BK, 1), (2 * BK, 1), (3 * BK, 1), (5 * BK, 2),
                          (65 * BK, 0), (65 * BK, 4)):
            for M in (8, tile + 8, 432):
                for N in (tile, 2 * tile):
                    cases.append((name, B, N, M, splitk))
        cases.append((name, 65536, tile, 8, 0))
    return cases


@requires_gpu
def test_mirror_matches_the_kernel_constants():
    lay = dict(ops._C.wgrad_glds_layout())
    assert list(lay.pop("off")) == wi.off_table()
    lay.pop("glds_default")
    assert lay == wi.LAYOUT


@requires_gpu
@pytest.mark.parametrize("name,B,N,M,splitk", _cases())
def test_glds_equals_regstage(name, B, N, M, splitk):
    kernel = getattr(ops._C, name)
    dy, x = _operands(B, N, M, seed=B + N + M + splitk)
    for out_bf16 in (False, True):
        new = kernel(dy, x, splitk, out_bf16, False)
        ctl = kernel(dy, x, splitk, out_bf16, True)
        assert new.shape == (N, M)
        assert new.dtype == (torch.bfloat16 if out_bf16 else torch.float32)
        assert torch.isfinite(new.float()).all()
        assert torch.equal(new, ctl)
    # the default is one of the two
    assert torch.equal(kernel(dy, x, splitk), kernel(dy, x, splitk, False,
                                                     True))


@requires_gpu
@pytest.mark.parametrize("name,tile", KERNELS)
def test_race_screen(name, tile):
    """An early read of a DMA target passes single runs; fifty launches on
    fixed inputs must all give the first launch's bits and the control's."""
    kernel = getattr(ops._C, name)
    dy, x = _operands(65 * BK, 2 * tile, 432, seed=tile)
    ctl = kernel(dy, x, 0, False, True)
    outs = [kernel(dy, x, 0, False, False) for _ in range(50)]
    torch.cuda.synchronize()
    assert torch.equal(outs[0], ctl)
    for out in outs[1:]:
        assert torch.equal(out, outs[0])


@requires_gpu
def test_linear_wgrad_env_switch(monkeypatch):
    dz, x = _operands(320, 256, 432, seed=7)
    weight = torch.empty(256, 432, dtype=torch.bfloat16, device="cuda")
    assert ops._custom_wgrad_kernel(dz, x) is not None
    monkeypatch.delenv("MIYARN_WGRAD", raising=False)
    new = ops._linear_wgrad(dz, x, weight)
    monkeypatch.setenv("MIYARN_WGRAD", "regstage")
    ctl = ops._linear_wgrad(dz, x, weight)
    assert new.dtype == ctl.dtype == torch.bfloat16
    assert torch.equal(new, ctl)
    # and the env route is the explicit control
    kernel = ops._custom_wgrad_kernel(dz, x)
    assert torch.equal(ctl, kernel(dz, x, 0, True, True))
