"""The narrow-output split-K weight-gradient kernel
(``csrc/wgrad_narrow.hip``) against float64 ``dy.T @ x``: 128 wide columns
per block, the narrow side padded to 32, 64 or 128, 64-row k-steps with a
zero-filled k tail, fp32 slabs summed by ``reduce_splitk``."""

import pytest
import torch

import cross_lowrank_ref as R
import exact_ints
from tf_yarn_amd import ops

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X"),
]

BF16 = torch.bfloat16


def _check(dy, x, splitk=0):
    """Both output types of one exact case against the float64 product."""
    ref = dy.double().t() @ x.double()
    dyg, xg = dy.to(BF16).cuda(), x.to(BF16).cuda()
    got = ops._C.wgrad_narrow(dyg, xg, splitk, False).cpu()
    assert got.dtype == torch.float32 and torch.equal(got, ref.float())
    got = ops._C.wgrad_narrow(dyg, xg, splitk, True).cpu()
    assert got.dtype == BF16 and torch.equal(got, exact_ints.rne_bf16(ref))


# (r, Wd, B): every value of each axis, in both orientations below
SHAPES = [(8, 8, 1), (8, 48, 65), (16, 136, 63), (16, 432, 300),
          (48, 48, 64), (48, 528, 1), (64, 432, 65), (64, 136, 300),
          (128, 528, 63), (128, 432, 64), (128, 136, 300)]


@pytest.mark.parametrize("narrow_is_n", [True, False])
@pytest.mark.parametrize("r,wd,b", SHAPES)
def test_exact(r, wd, b, narrow_is_n):
    n, m = (r, wd) if narrow_is_n else (wd, r)
    _check(*exact_ints.operands((b, n), (b, m), b, seed=r + wd + b))


@pytest.mark.parametrize("b,splitk,n,m", [
    (192, 2, 64, 432),      # 2 + 1 k-steps
    (4164, 4, 432, 64),     # a short, ragged last slab
    (192, 100, 432, 64),    # clamped by the host to one step per slab
    (4164, 0, 64, 432),     # the auto plan
    (65536, 0, 432, 64),    # the workload's depth
])
def test_split_plan(b, splitk, n, m):
    _check(*exact_ints.operands((b, n), (b, m), b, seed=b + splitk), splitk)


@pytest.mark.parametrize("n,m", [(432, 64), (64, 432)])
def test_position_coded(n, m):
    """``dy`` has a single 1 per column, at row ``b0(n)``; ``x[b, m]`` is a
    code of ``(b, m)``: every output entry names where it came from."""
    b = 300
    b0 = (torch.arange(n) * 7 + 3) % b
    dy = torch.zeros(b, n)
    dy[b0, torch.arange(n)] = 1
    # 509 values k / 4, |k| <= 254: 8 significant bits at most
    code = (torch.arange(b)[:, None] * 31 + torch.arange(m)[None, :] * 17)
    x = (code % 509 - 254).float() / 4
    assert torch.equal(x.to(BF16).float(), x) and x.unique().numel() > 500
    got = ops._C.wgrad_narrow(dy.to(BF16).cuda(), x.to(BF16).cuda()).cpu()
    assert torch.equal(got, x[b0])


def test_real_roundings():
    b, n, m = 129, 48, 432
    exact_ints.assert_exact(16, 16, b)
    gen = torch.Generator().manual_seed(5)
    dy, x = exact_ints.ints((b, n), 16, gen), exact_ints.ints((b, m), 16, gen)
    ref = dy.double().t() @ x.double()
    err = (exact_ints.rne_bf16(ref).double() - ref).abs()
    assert (err != 0).any(), "nothing to round"
    assert ((err != 0) & (err == exact_ints.bf16_half_ulp(ref))).any(), \
        "no tie"
    got = ops._C.wgrad_narrow(dy.to(BF16).cuda(), x.to(BF16).cuda(), 0, True)
    assert torch.equal(got.cpu(), exact_ints.rne_bf16(ref))


def test_bounded():
    """One bf16 rounding plus the fp32 error of a length-``b`` sum."""
    b, n, m = 257, 432, 112
    gen = torch.Generator().manual_seed(1)
    dy = torch.randn(b, n, generator=gen).to(BF16)
    x = torch.randn(b, m, generator=gen).to(BF16)
    ref = dy.double().t() @ x.double()
    mag = dy.double().abs().t() @ x.double().abs()
    got = ops._C.wgrad_narrow(dy.cuda(), x.cuda(), 0, True).cpu()
    err = (got.double() - ref).abs()
    bound = exact_ints.bf16_half_ulp(ref) + (b + 2) * 2.0 ** -23 * mag
    print(f"max err / bound = {(err / bound.clamp_min(1e-300)).max():.3f}")
    assert (err <= bound).all()


def test_routing_through_the_public_op(monkeypatch):
    b, d, r = 129, 48, 16
    cpu = [a.to(BF16) for a in R.int_operands(b, d, r, seed=4)]
    want = R.ref64(*cpu)
    calls = []
    fn = ops._C.wgrad_narrow
    monkeypatch.setattr(ops._C, "wgrad_narrow",
                        lambda *a: calls.append(fn(*a)) or calls[-1])

    def step():
        leaves = [a.cuda().requires_grad_() for a in cpu[:5]]
        y = ops.cross_layer_lowrank(*leaves)
        t = y.grad_fn.saved_tensors[4]
        assert ops._custom_wgrad_kernel(cpu[5].cuda(), t) is None
        _, _, dv, du, _ = torch.autograd.grad(y, leaves, cpu[5].cuda())
        return du.cpu(), dv.cpu()

    du, dv = step()
    assert [tuple(c.shape) for c in calls] == [(r, d), (d, r)]
    assert torch.equal(du, exact_ints.rne_bf16(want[R.NAMES.index("dU")]))
    assert torch.equal(dv, exact_ints.rne_bf16(want[R.NAMES.index("dV")]))
    monkeypatch.setenv("MIYARN_WGRAD", "lib")
    du_lib, dv_lib = step()
    assert len(calls) == 2
    assert torch.equal(du_lib, du) and torch.equal(dv_lib, dv)


@pytest.mark.parametrize("n,m,dtype", [(136, 432, BF16), (64, 436, BF16),
                                       (64, 432, torch.float32)])
def test_refusals(n, m, dtype):
    dy, x = exact_ints.operands((65, n), (65, m), 65, seed=n + m)
    dy, x = dy.to(dtype).cuda(), x.to(dtype).cuda()
    with pytest.raises(RuntimeError, match="wgrad_narrow"):
        ops._C.wgrad_narrow(dy, x)
    assert not ops._narrow_wgrad_ok(dy, x)
    w = torch.empty(n, m, dtype=dtype, device="cuda")
    assert torch.equal(ops._linear_wgrad(dy, x, w), dy.t().matmul(x))
