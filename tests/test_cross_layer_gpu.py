"""The cross-layer HIP kernels (``csrc/cross_layer.hip``) against the
float64 definition, through the public op and autograd.

Exact cases: integer operands (``cross_layer_ref.int_operands``), so every
fp32 intermediate is exact in any order and all six results must be
``rne_bf16`` of the float64 ones bit for bit.  The forward tile is 128 x
128 with 64-wide k-steps: ``D`` = 16, 48 (k tail, ragged column tile), 64,
144 (second column tile, three k-steps with a 16 tail), 432, 528 (five
column tiles) and ``B`` = 1, 5, 129 (second row tile of one row), 300."""

import pytest
import torch

import cross_layer_ref as R
import exact_ints
from dot_interaction_ref import pitched
from tf_yarn_amd import ops
from tf_yarn_amd.models import DCN

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X"),
]

BF16 = torch.bfloat16


def _run(x0, x, w, bias, g, loss=None):
    """(y, v, dx0, dx, dW, dbias) on the CPU from the public op and
    autograd; ``v`` is the one the forward binding saved.  ``loss(y)``
    replaces the backward from ``g``."""
    x0, x, w, bias = (t.cuda().requires_grad_() for t in (x0, x, w, bias))
    assert ops.cross_layer_kernel_ok(x0, x, w, bias)
    y = ops.cross_layer(x0, x, w, bias)
    v = y.grad_fn.saved_tensors[3]
    if loss is None:
        grads = torch.autograd.grad(y, (x0, x, w, bias), g.cuda())
    else:
        grads = torch.autograd.grad(loss(y), (x0, x, w, bias))
    return [t.detach().cpu() for t in (y, v, *grads)]


def _assert_exact(got, want):
    for name, a, r in zip(R.NAMES, got, want):
        w = exact_ints.rne_bf16(r)
        assert a.dtype == BF16 and a.shape == w.shape, name
        assert torch.equal(a, w), name


@pytest.mark.parametrize("b", [1, 5, 129, 300])
@pytest.mark.parametrize("d", [16, 48, 64, 144, 432, 528])
def test_exact(d, b):
    ops_ = [t.to(BF16) for t in R.int_operands(b, d, seed=b + d)]
    _assert_exact(_run(*ops_), R.ref64(*ops_))


@pytest.mark.parametrize("b,d", [(129, 48), (300, 144)])
def test_exact_rounds(b, d):
    """Operands in [-16, 16]: what catches ``y`` from the rounded ``v``, a
    double rounding of ``dz @ W + g``, or truncation."""
    ops_ = [t.to(BF16) for t in R.int_operands(b, d, seed=1, amax=16)]
    ref = R.ref64(*ops_)
    for name in ("y", "dx", "dx0"):
        r = ref[R.NAMES.index(name)]
        err = (exact_ints.rne_bf16(r).double() - r).abs()
        assert (err != 0).any(), f"{name}: nothing to round"
        assert ((err != 0) & (err == exact_ints.bf16_half_ulp(r))).any(), \
            f"{name}: no tie"
    _assert_exact(_run(*ops_), ref)


def _assert_bounded(x0, x, w, bias, g, got):
    """``got`` within one correct bf16 rounding plus the worst fp32
    accumulation error of a length-``k`` sum of the float64 definition;
    the backward's reference takes the kernel's own ``v``."""
    b, d = x.shape
    v = got[1]
    want = R.ref64(x0, x, w, bias, g, v)
    mags = R.ref64(x0.abs(), x.abs(), w.abs(), bias.abs(), g.abs(), v.abs())
    for name, a, r, mag, k in zip(R.NAMES, got, want, mags,
                                  (d, d, 1, d, b, b)):
        err = (a.double() - r).abs()
        bound = exact_ints.bf16_half_ulp(r) + (k + 2) * 2.0 ** -23 * mag
        print(f"{name}: max err / bound = "
              f"{(err / bound.clamp_min(1e-300)).max():.3f}")
        assert (err <= bound).all(), name


@pytest.mark.parametrize("b,d", [(257, 432), (9, 528)])
def test_bounded(b, d):
    gen = torch.Generator().manual_seed(1)
    x0, x, g = (torch.randn(b, d, generator=gen).to(BF16) for _ in range(3))
    w = (torch.randn(d, d, generator=gen) * d ** -0.5).to(BF16)
    bias = torch.randn(d, generator=gen).to(BF16)
    _assert_bounded(x0, x, w, bias, g, _run(x0, x, w, bias, g))


def test_three_row_pitches_give_the_same_bits():
    """``x0``, ``x`` and ``grad_y`` as views of buffers 8, 16 and 24 columns
    wider, the gaps full of NaN: a read at the wrong pitch or past a row's
    end shows."""
    b, d = 9, 48
    x0, x, w, bias, g = (t.to(BF16) for t in R.int_operands(b, d, seed=6))
    want = _run(x0, x, w, bias, g)
    _assert_exact(want, R.ref64(x0, x, w, bias, g))
    views = [pitched(t.cuda(), d + extra)
             for t, extra in ((x0, 8), (x, 16), (g, 24))]
    assert [v.stride(0) for v in views] == [d + 8, d + 16, d + 24]
    assert ops._C.cross_rows_ok(views[2])
    got = _run(views[0], views[1], w, bias, views[2])
    for name, a, c in zip(R.NAMES, got, want):
        assert torch.equal(a, c), name


@pytest.mark.parametrize("case", ["sum_over_batch", "sum_of_all"])
def test_grad_y_from_autograd(case):
    """A reduction over the batch hands the backward a ``grad_y`` with row
    stride 0, which the binding refuses: the op copies it."""
    b, d = 9, 48
    x0, x, w, bias, g = (t.to(BF16) for t in R.int_operands(b, d, seed=8))
    if case == "sum_over_batch":
        g = g[:1].expand(b, -1)  # integers in [-2, 2]
        got = _run(x0, x, w, bias, g,
                   lambda y: (y.sum(0) * g[0].cuda()).sum())
    else:
        g = torch.ones_like(g)
        got = _run(x0, x, w, bias, g, lambda y: y.sum())
    _assert_exact(got, R.ref64(x0, x, w, bias, g))


def test_empty_batch():
    d = 48
    x0, x = (torch.zeros(0, d, dtype=BF16, device="cuda", requires_grad=True)
             for _ in range(2))
    w = torch.ones(d, d, dtype=BF16, device="cuda", requires_grad=True)
    bias = torch.ones(d, dtype=BF16, device="cuda", requires_grad=True)
    assert ops.cross_layer_kernel_ok(x0, x, w, bias)
    y = ops.cross_layer(x0, x, w, bias)
    assert y.shape == (0, d) and y.dtype == BF16
    grads = torch.autograd.grad(y, (x0, x, w, bias), torch.zeros_like(y))
    torch.cuda.synchronize()
    assert [t.shape for t in grads] == [(0, d), (0, d), (d, d), (d,)]
    assert not grads[2].any() and not grads[3].any()


def test_no_grad_saves_no_v(monkeypatch):
    b, d = 129, 144
    x0, x, w, bias, _ = (t.to(BF16).cuda()
                         for t in R.int_operands(b, d, seed=3))
    w.requires_grad_()
    results = []
    fwd = ops._C.cross_fwd
    monkeypatch.setattr(ops._C, "cross_fwd", lambda *a: results.append(
        fwd(*a)) or results[-1])
    y_train = ops.cross_layer(x0, x, w, bias)
    with torch.no_grad():
        y_eval = ops.cross_layer(x0, x, w, bias)
    (_, v_train), (_, v_eval) = results
    assert v_train is not None and v_eval is None
    assert torch.equal(y_train, y_eval)


# ---- DCN on the GPU --------------------------------------------------------

SIZES = [7, 5, 3]


def _dcn_step(monkeypatch):
    """One bf16 training step of a small DCN, one-hot.  Returns the model,
    the hook's record of the second cross layer, the number of forward
    binding calls, the table before the step and the touched rows."""
    torch.manual_seed(0)
    m = DCN(table_sizes=SIZES, embedding_dim=16, n_cross=3, deep=(32, 16),
            compute_dtype=BF16).cuda()
    gen = torch.Generator().manual_seed(2)
    dense = torch.randn(8, m.dense_dim, generator=gen).cuda()
    labels = torch.tensor([0., 1., 1., 0.] * 2).cuda()
    ids = torch.tensor([[0, 1, 2], [6, 4, 0], [3, 3, 1], [0, 0, 2]] * 2)
    touched = (ids + m.embedding.offsets.cpu()).reshape(-1)
    seen, calls = [], []
    m.cross.layers[1].register_forward_hook(
        lambda mod, args, out: seen.append((*args, out)))
    fwd = ops._C.cross_fwd
    monkeypatch.setattr(ops._C, "cross_fwd",
                        lambda *a: calls.append(1) or fwd(*a))
    before = m.embedding.weight.detach().cpu()
    loss = m(dense, ids.cuda(), labels)
    loss.backward()
    assert torch.isfinite(loss).item()
    m.apply_sparse_updates(0.1)
    return m, seen, len(calls), before, touched


def test_dcn_step_runs_the_kernel_on_its_own_tensors(monkeypatch):
    m, seen, n_calls, before, touched = _dcn_step(monkeypatch)
    assert n_calls == 3
    (x0, x, y), = seen
    layer = m.cross.layers[1]
    assert x0.shape == (8, 64) and x.abs().sum() > 0
    assert ops.cross_layer_kernel_ok(x0, x, layer.weight, layer.bias)
    args = [t.detach().cpu() for t in (x0, x, layer.weight, layer.bias)]
    want = R.ref64(*args, torch.zeros(8, 64))[0]
    mag = R.ref64(*(t.abs() for t in args), torch.zeros(8, 64))[0]
    err = (y.detach().cpu().double() - want).abs()
    bound = exact_ints.bf16_half_ulp(want) + (64 + 2) * 2.0 ** -23 * mag
    print(f"y: max err / bound = "
          f"{(err / bound.clamp_min(1e-300)).max():.3f}")
    assert (err <= bound).all()
    for p in layer.parameters():
        assert p.grad is not None and p.grad.abs().sum() > 0

    after = m.embedding.weight.detach().cpu()
    is_touched = torch.zeros(sum(SIZES), dtype=torch.bool)
    is_touched[touched] = True
    assert not is_touched.all() and (after != before).any()
    assert torch.equal(after[~is_touched], before[~is_touched])


def test_dcn_switched_off_calls_no_binding(monkeypatch):
    monkeypatch.setenv("MIYARN_CROSS_LAYER", "0")
    assert _dcn_step(monkeypatch)[2] == 0
