"""The dot-interaction HIP kernels (``csrc/dot_interaction.hip``) against
the float64 definition.

Exact cases: integer operands in [-2, 2] (``exact_ints``), so every dot
product and every ``S @ T`` entry is exact in fp32 in any order and the
kernels must give ``rne_bf16`` of the float64 result bit for bit: the
pass-through and pad columns, the packed triangle, both gradients.  The
bounded case uses N(0, 1) operands and the derived bound of one correct
bf16 rounding plus the worst fp32 accumulation error of a length-``K`` sum.

A wave takes one example and a block four per trip: ``B = 15`` with
``max_blocks=2`` gives both blocks two trips and the last one a ragged
group of three."""

import pytest
import torch

import dot_interaction_ref as R
import exact_ints
from tf_yarn_amd import ops

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X"),
]

BF16 = torch.bfloat16


def _kernels(dv, emb, g, max_blocks=0):
    """(out, d_dense_vec, d_emb) on the CPU: through the public op and
    autograd, or through the bindings when the grid is capped."""
    dv, emb, g = (t.cuda() for t in (dv, emb, g))
    if max_blocks:
        out = ops._C.dot_interaction_fwd(dv, emb, max_blocks)
        grads = ops._C.dot_interaction_bwd(g, dv, emb, max_blocks)
    else:
        assert ops.dot_interaction_kernel_ok(dv, emb)
        dv.requires_grad_()
        emb.requires_grad_()
        out = ops.dot_interaction(dv, emb)
        grads = torch.autograd.grad(out, (dv, emb), g)
    return [t.detach().cpu() for t in (out, *grads)]


@pytest.mark.parametrize("b,max_blocks", [(1, 0), (5, 0), (15, 2)])
@pytest.mark.parametrize("n,d", [(2, 16), (3, 16), (27, 16), (32, 16),
                                 (27, 32), (5, 128)])
def test_exact(n, d, b, max_blocks):
    dv, emb, g = (t.to(BF16) for t in R.int_operands(b, n, d, seed=n + d))
    want = [exact_ints.rne_bf16(t) for t in R.ref64(dv, emb, g)]
    if d == 128:  # the rounding itself is under test
        assert R.ref64(dv, emb)[0, d] == 509 and want[0][0, d] == 508
    got = _kernels(dv, emb, g, max_blocks)
    for name, a, w in zip(("out", "d_dense_vec", "d_emb"), got, want):
        assert a.shape == w.shape and torch.equal(a, w), name


def test_bounded():
    n, d, b = 27, 16, 257
    gen = torch.Generator().manual_seed(1)
    dv = torch.randn(b, d, generator=gen).to(BF16)
    emb = torch.randn(b, (n - 1) * d, generator=gen).to(BF16)
    g = torch.randn(b, ops.dot_interaction_width(n - 1, d),
                    generator=gen).to(BF16)
    want = R.ref64(dv, emb, g)
    # sum_k |a_k * b_k| of every element: the same sums over magnitudes
    # (a copied column is no sum; d_dense_vec's includes its |g| term)
    mags = list(R.ref64(dv.abs(), emb.abs(), g.abs()))
    mags[0][:, :d] = 0
    got = _kernels(dv, emb, g)
    for name, a, w, mag, k in zip(("out", "d_dense_vec", "d_emb"), got, want,
                                  mags, (d, n, n)):
        err = (a.double() - w).abs()
        bound = exact_ints.bf16_half_ulp(w) + k * 2.0 ** -23 * mag
        print(f"{name}: max err / bound = {(err / bound.clamp_min(1e-300)).max():.3f}")
        assert (err <= bound).all(), name


def test_strided_emb_gives_the_same_bits():
    n, d, b = 27, 16, 9
    dv, emb, g = (t.to(BF16) for t in R.int_operands(b, n, d, seed=3))
    wide = torch.zeros(b, emb.shape[1] + 16, dtype=BF16, device="cuda")
    wide[:, :emb.shape[1]] = emb.cuda()
    view = wide[:, :emb.shape[1]]
    assert view.stride(0) == emb.shape[1] + 16
    for a, w in zip(_kernels(dv, view, g), _kernels(dv, emb, g)):
        assert torch.equal(a, w)


@pytest.mark.parametrize("case", ["odd_offset", "n33", "d8"])
def test_refused_operands_take_the_composition(case):
    n, d = {"odd_offset": (27, 16), "n33": (33, 16), "d8": (4, 8)}[case]
    dv, emb, g = (t.to(BF16) for t in R.int_operands(5, n, d, seed=4))
    want = [exact_ints.rne_bf16(t) for t in R.ref64(dv, emb, g)]
    dv, emb, g = dv.cuda(), emb.cuda(), g.cuda()
    if case == "odd_offset":
        flat = torch.zeros(emb.numel() + 1, dtype=BF16, device="cuda")
        flat[1:] = emb.reshape(-1)
        emb = flat[1:].view_as(emb)
    assert not ops.dot_interaction_kernel_ok(dv, emb)
    dv.requires_grad_()
    emb.requires_grad_()
    out = ops.dot_interaction(dv, emb)
    got = [out, *torch.autograd.grad(out, (dv, emb), g)]
    for a, w in zip(got, want):
        assert torch.equal(a.cpu(), w)
