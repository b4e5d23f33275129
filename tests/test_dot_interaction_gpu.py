"""The dot-interaction HIP kernels (``csrc/dot_interaction.hip``) against
the float64 definition.

Exact cases: integer operands (``exact_ints``), so every dot product and
every ``S @ T`` entry is exact in fp32 in any order and the kernels must
give ``rne_bf16`` of the float64 result bit for bit: the pass-through and
pad columns, the packed triangle, both gradients.  In [-2, 2] every result
is an integer that bf16 holds (but for one planted 509); in [-16, 16] a
quarter to a half of the results are rounded, exact ties among them.  The
bounded cases use N(0, 1) operands, or the DLRM model's own tensors, and
the derived bound of one correct bf16 rounding plus the worst fp32
accumulation error of a length-``K`` sum.

A wave takes one example and a block four per trip: ``B = 15`` with
``max_blocks=2`` gives both blocks two trips and the last one a ragged
group of three.  A lane writes the output row's columns ``8 * lane ..`` and,
for ``W > 512`` only, ``8 * (lane + 64) ..``."""

import pytest
import torch

import dot_interaction_ref as R
import exact_ints
from tf_yarn_amd import ops
from tf_yarn_amd.models import DLRM

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X"),
]

BF16 = torch.bfloat16
NAMES = ("out", "d_dense_vec", "d_emb")


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


def _want(dv, emb, g):
    return [exact_ints.rne_bf16(t) for t in R.ref64(dv, emb, g)]


# the second group: rows wider than 512 columns (the lanes' second chunk)
# and the row pitches 96, 160 and 224 bytes of the backward's LDS image
EXACT_SHAPES = [(2, 16), (3, 16), (27, 16), (32, 16), (27, 32), (5, 128),
                (32, 32), (31, 64), (32, 48), (27, 80), (32, 112), (32, 128)]


@pytest.mark.parametrize("b,max_blocks", [(1, 0), (5, 0), (15, 2)])
@pytest.mark.parametrize("n,d", EXACT_SHAPES)
def test_exact(n, d, b, max_blocks):
    assert sum(ops.dot_interaction_width(n_ - 1, d_) > 512
               for n_, d_ in EXACT_SHAPES) >= 3
    dv, emb, g = (t.to(BF16) for t in R.int_operands(b, n, d, seed=n + d))
    want = _want(dv, emb, g)
    if d == 128:  # the rounding itself is under test
        assert R.ref64(dv, emb)[0, d] == 509 and want[0][0, d] == 508
    got = _kernels(dv, emb, g, max_blocks)
    for name, a, w in zip(NAMES, got, want):
        assert a.shape == w.shape and torch.equal(a, w), name


@pytest.mark.parametrize("n,d", [(27, 16), (32, 32), (32, 48), (32, 128)])
def test_exact_rounds(n, d):
    """Operands in [-16, 16]: still exact in fp32 in any order, but the
    results no longer fit bf16, so the one rounding of each output (and of
    ``float(g) + dT`` as a whole) is what the comparison sees."""
    dv, emb, g = (t.to(BF16) for t in R.int_operands(15, n, d, seed=1,
                                                     amax=16))
    ref = R.ref64(dv, emb, g)
    want = [exact_ints.rne_bf16(t) for t in ref]
    for name, r, w in zip(NAMES, ref, want):
        err = (w.double() - r).abs()
        assert (err != 0).any(), f"{name}: nothing to round"
        assert ((err != 0) & (err == exact_ints.bf16_half_ulp(r))).any(), \
            f"{name}: no tie"
    got = _kernels(dv, emb, g, max_blocks=2)
    for name, a, w in zip(NAMES, got, want):
        assert a.shape == w.shape and torch.equal(a, w), name


def _assert_bounded(dv, emb, g, got):
    """``got`` within one correct bf16 rounding plus the worst fp32
    accumulation error of a length-``k`` sum of the float64 definition."""
    d = dv.shape[1]
    n = emb.shape[1] // d + 1
    want = R.ref64(dv, emb, g)
    # sum_k |a_k * b_k| of every element: the same sums over magnitudes
    # (a copied column is no sum; d_dense_vec's includes its |g| term)
    mags = list(R.ref64(dv.abs(), emb.abs(), g.abs()))
    mags[0][:, :d] = 0
    for name, a, w, mag, k in zip(NAMES, got, want, mags, (d, n, n)):
        err = (a.double() - w).abs()
        bound = exact_ints.bf16_half_ulp(w) + k * 2.0 ** -23 * mag
        print(f"{name}: max err / bound = {(err / bound.clamp_min(1e-300)).max():.3f}")
        assert (err <= bound).all(), name


@pytest.mark.parametrize("n,d,b", [(27, 16, 257), (32, 128, 9)])
def test_bounded(n, d, b):
    gen = torch.Generator().manual_seed(1)
    dv = torch.randn(b, d, generator=gen).to(BF16)
    emb = torch.randn(b, (n - 1) * d, generator=gen).to(BF16)
    g = torch.randn(b, ops.dot_interaction_width(n - 1, d),
                    generator=gen).to(BF16)
    _assert_bounded(dv, emb, g, _kernels(dv, emb, g))


def test_strided_emb_gives_the_same_bits():
    n, d, b = 27, 16, 9
    dv, emb, g = (t.to(BF16) for t in R.int_operands(b, n, d, seed=3))
    wide = torch.zeros(b, emb.shape[1] + 16, dtype=BF16, device="cuda")
    wide[:, :emb.shape[1]] = emb.cuda()
    view = wide[:, :emb.shape[1]]
    assert view.stride(0) == emb.shape[1] + 16
    for a, w in zip(_kernels(dv, view, g), _kernels(dv, emb, g)):
        assert torch.equal(a, w)


@pytest.mark.parametrize("n,d", [(27, 16), (32, 48)])
def test_three_row_pitches_give_the_same_bits(n, d):
    """``dense_vec``, ``emb`` and ``grad_out`` as views of wider buffers,
    each at its own pitch, the gaps full of NaN: a read at the wrong pitch
    or past a row's end shows."""
    b = 9
    dv, emb, g = (t.to(BF16) for t in R.int_operands(b, n, d, seed=6))
    want = _want(dv, emb, g)
    views = [R.pitched(t.cuda(), t.shape[1] + extra)
             for t, extra in ((dv, 8), (emb, 16), (g, 24))]
    assert len({v.stride(0) - v.shape[1] for v in views}) == 3
    assert ops.dot_interaction_kernel_ok(*views[:2])
    assert ops._C.dot_interaction_grad_ok(views[2])
    out = ops._C.dot_interaction_fwd(*views[:2])
    got = [out, *ops._C.dot_interaction_bwd(views[2], *views[:2])]
    for name, a, c, w in zip(NAMES, got, _kernels(dv, emb, g), want):
        assert torch.equal(a.cpu(), c), name
        assert torch.equal(c, w), name


class _Recorded:
    """A binding that keeps every call's tensor arguments and results."""

    def __init__(self, fn):
        self.fn, self.calls = fn, []

    def __call__(self, *args):
        res = self.fn(*args)
        outs = [res] if isinstance(res, torch.Tensor) else list(res)
        self.calls.append(([a for a in args if isinstance(a, torch.Tensor)],
                           outs))
        return res


class _GradAs(torch.autograd.Function):
    """The identity, whose backward hands on ``grad`` itself, layout and
    all, in place of the gradient it receives."""

    @staticmethod
    def forward(ctx, x, grad):
        ctx.grad = grad
        return x.view_as(x)

    @staticmethod
    def backward(ctx, _):
        return ctx.grad, None


def _leaves(b, n, d, seed):
    dv, emb, g = (t.to(BF16) for t in R.int_operands(b, n, d, seed=seed))
    dv_g = dv.cuda().requires_grad_()
    emb_g = emb.cuda().requires_grad_()
    assert ops.dot_interaction_kernel_ok(dv_g, emb_g)
    return dv, emb, g, dv_g, emb_g


@pytest.mark.parametrize("case", ["sum_over_batch", "sum_of_all"])
def test_expanded_grad_out(case, monkeypatch):
    """A reduction over the batch axis hands the backward a ``grad_out``
    with row stride 0.  The binding refuses such rows, so the op copies."""
    b, n, d = 9, 27, 16
    dv, emb, g, dv_g, emb_g = _leaves(b, n, d, seed=8)
    bwd = _Recorded(ops._C.dot_interaction_bwd)
    monkeypatch.setattr(ops._C, "dot_interaction_bwd", bwd)
    out = ops.dot_interaction(dv_g, emb_g)
    if case == "sum_over_batch":
        w = g[0]  # integers in [-2, 2], as int_operands checked
        (out.sum(0) * w.cuda()).sum().backward()
    else:
        w = torch.ones_like(g[0])
        out.sum().backward()
    want = _want(dv, emb, w.expand(b, -1))
    (seen, _), = bwd.calls
    assert ops._C.dot_interaction_grad_ok(seen[0])
    assert torch.equal(seen[0].cpu(), w.to(BF16).expand(b, -1))
    assert torch.equal(dv_g.grad.cpu(), want[1])
    assert torch.equal(emb_g.grad.cpu(), want[2])


@pytest.mark.parametrize("case", ["pitched", "odd_offset", "expanded"])
def test_grad_out_is_copied_only_when_the_binding_would_refuse_it(
        case, monkeypatch):
    b, n, d = 9, 27, 16
    dv, emb, g, dv_g, emb_g = _leaves(b, n, d, seed=9)
    if case == "pitched":
        g_dev = R.pitched(g.cuda(), g.shape[1] + 8)
    elif case == "odd_offset":
        flat = torch.full((g.numel() + 1,), float("nan"), dtype=BF16,
                          device="cuda")
        flat[1:] = g.cuda().reshape(-1)
        g_dev = flat[1:].view_as(g)
        assert g_dev.data_ptr() % 16 == 2
    else:
        g = g[:1].expand(b, -1)
        g_dev = g[:1].cuda().expand(b, -1)
        assert g_dev.stride() == (0, 1)
    legal = case == "pitched"
    assert ops._C.dot_interaction_grad_ok(g_dev) == legal
    want = _want(dv, emb, g)
    bwd = _Recorded(ops._C.dot_interaction_bwd)
    monkeypatch.setattr(ops._C, "dot_interaction_bwd", bwd)
    out = _GradAs.apply(ops.dot_interaction(dv_g, emb_g), g_dev)
    out.sum().backward()
    (seen, _), = bwd.calls
    if legal:
        assert seen[0].data_ptr() == g_dev.data_ptr()
        assert seen[0].stride() == g_dev.stride()
    else:
        assert seen[0].data_ptr() != g_dev.data_ptr()
        assert seen[0].is_contiguous() and seen[0].data_ptr() % 16 == 0
    assert torch.equal(dv_g.grad.cpu(), want[1])
    assert torch.equal(emb_g.grad.cpu(), want[2])


@pytest.mark.parametrize("where", ["emb", "grad_out"])
def test_non_finite_values_stay_in_their_example(where):
    """One block, trips of 4 + 4 + 1 examples: example 1 is poisoned,
    example 5 is the same wave's next trip, the others are its neighbours'.
    All of them must be bit-identical to the clean run.  Inside example 1
    the kernels sum ``S[k][i] * T[k][c]`` over all k, zeros included, as
    the float64 definition does: NaN where it has NaN, the same signed Inf
    elsewhere."""
    n, d, b = 27, 16, 9
    dv, emb, g = (t.to(BF16) for t in R.int_operands(b, n, d, seed=5))
    clean = _kernels(dv, emb, g, max_blocks=1)
    if where == "emb":
        emb = R.poison_emb(emb, d)
    else:
        g = R.poison_grad(g, d)
    want = _want(dv, emb, g)
    got = _kernels(dv, emb, g, max_blocks=1)
    others = [i for i in range(b) if i != 1]
    for name, a, c, w in zip(NAMES, got, clean, want):
        assert torch.equal(a[others], c[others]), name
        assert torch.equal(a[others], w[others]), name
    assert not all(w[1].isfinite().all() for w in want[1:])
    for name, a, w in zip(NAMES, got, want):
        print(f"{name}[1]: {int(w[1].isnan().sum())} NaN, "
              f"{int(w[1].isinf().sum())} Inf in the reference; "
              f"{int(a[1].isnan().sum())} NaN, {int(a[1].isinf().sum())} Inf "
              f"from the kernel")
        assert torch.equal(a[1].isnan(), w[1].isnan()), name
        assert R.same_bits(a[1], w[1]), name


def test_empty_batch():
    n, d = 27, 16
    dv = torch.zeros(0, d, dtype=BF16, device="cuda", requires_grad=True)
    emb = torch.zeros(0, (n - 1) * d, dtype=BF16, device="cuda",
                      requires_grad=True)
    assert ops.dot_interaction_kernel_ok(dv, emb)
    out = ops.dot_interaction(dv, emb)
    w = ops.dot_interaction_width(n - 1, d)
    assert out.shape == (0, w) and out.dtype == BF16
    d_dv, d_emb = torch.autograd.grad(out, (dv, emb), torch.zeros_like(out))
    torch.cuda.synchronize()
    assert d_dv.shape == (0, d) and d_emb.shape == (0, (n - 1) * d)


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


# ---- DLRM on the GPU -------------------------------------------------------

SIZES = [7, 5, 3]


def _dlrm_batch(m, multi_hot):
    """The id patterns of the CPU test (test_dot_interaction.py), twice:
    ``B = 8``.  Returns the model's arguments on the GPU and the table rows
    the batch touches."""
    b = 8
    gen = torch.Generator().manual_seed(2)
    dense = torch.randn(b, m.dense_dim, generator=gen)
    labels = torch.tensor([0., 1., 1., 0.] * 2)
    offs = m.embedding.offsets.cpu()
    if multi_hot:
        lens = torch.tensor([1, 2, 0, 3, 1, 1, 2, 2, 1, 0, 1, 2] * 2)
        bag_offsets = torch.cat([lens.new_zeros(1), lens.cumsum(0)]).cuda()
        feat = torch.repeat_interleave(torch.arange(b * 3) % 3, lens)
        ids = torch.tensor([3, 1, 4, 0, 1, 6, 2, 2, 6, 2, 1, 0, 1, 4, 0, 2]
                           * 2)
        touched = ids + offs[feat]
    else:
        bag_offsets = None
        ids = torch.tensor([[0, 1, 2], [6, 4, 0], [3, 3, 1], [0, 0, 2]] * 2)
        touched = (ids + offs).reshape(-1)
    return (dense.cuda(), ids.cuda(), labels.cuda(), bag_offsets), touched


def _dlrm(dtype):
    torch.manual_seed(0)
    return DLRM(table_sizes=SIZES, embedding_dim=16, bottom=(16,), top=(16,),
                compute_dtype=dtype).cuda()


def _record_both(monkeypatch):
    fwd = _Recorded(ops._C.dot_interaction_fwd)
    bwd = _Recorded(ops._C.dot_interaction_bwd)
    monkeypatch.setattr(ops._C, "dot_interaction_fwd", fwd)
    monkeypatch.setattr(ops._C, "dot_interaction_bwd", bwd)
    return fwd, bwd


@pytest.mark.parametrize("multi_hot", [False, True])
def test_dlrm_step_runs_the_kernels_on_its_own_tensors(multi_hot,
                                                       monkeypatch):
    """One bf16 training step calls each kernel exactly once, so the bottom
    MLP's output, the embedding's output and the top MLP's gradient are
    layouts the kernels take; what the kernels made of them is within
    ``test_bounded``'s bound of the float64 definition."""
    m = _dlrm(BF16)
    (dense, ids, labels, bag_offsets), touched = _dlrm_batch(m, multi_hot)
    fwd, bwd = _record_both(monkeypatch)
    before = m.embedding.weight.detach().cpu()
    loss = m(dense, ids, labels, bag_offsets=bag_offsets)
    loss.backward()
    assert torch.isfinite(loss).item()
    assert len(fwd.calls) == 1 and len(bwd.calls) == 1
    ((dv, emb), (out,)), = fwd.calls
    ((g, dv_b, emb_b), grads), = bwd.calls
    assert ops.dot_interaction_kernel_ok(dv, emb)
    assert dv_b.data_ptr() == dv.data_ptr()
    assert emb_b.data_ptr() == emb.data_ptr()
    assert dv.shape == (8, 16) and emb.shape == (8, 48) and g.shape == (8, 32)
    assert g.abs().sum() > 0 and emb.abs().sum() > 0
    _assert_bounded(dv.detach().cpu(), emb.detach().cpu(), g.cpu(),
                    [t.detach().cpu() for t in (out, *grads)])

    m.apply_sparse_updates(0.1)
    after = m.embedding.weight.detach().cpu()
    is_touched = torch.zeros(sum(SIZES), dtype=torch.bool)
    is_touched[touched] = True
    assert not is_touched.all()
    changed = (after != before).any(1)
    assert torch.equal(after[~is_touched], before[~is_touched])
    assert torch.equal(changed, is_touched)


@pytest.mark.parametrize("case", ["switched_off", "fp32"])
def test_dlrm_without_the_kernels(case, monkeypatch):
    if case == "switched_off":
        monkeypatch.setenv("MIYARN_DOT_INTERACTION", "0")
    m = _dlrm(BF16 if case == "switched_off" else torch.float32)
    (dense, ids, labels, bag_offsets), _ = _dlrm_batch(m, False)
    fwd, bwd = _record_both(monkeypatch)
    loss = m(dense, ids, labels, bag_offsets=bag_offsets)
    loss.backward()
    assert torch.isfinite(loss).item()
    assert not fwd.calls and not bwd.calls
