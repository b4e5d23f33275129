"""The low-rank cross-layer HIP kernels (``csrc/cross_lowrank.hip``) against
the float64 definition, through the public op and autograd (128-row bands,
64-wide k-steps, 64-column tiles, the rank padded to 32, 64 or 128)."""

import pytest
import torch

import cross_lowrank_ref as R
import exact_ints
from dot_interaction_ref import pitched
from tf_yarn_amd import ops
from tf_yarn_amd.models import DCN

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X"),
]

BF16 = torch.bfloat16


def _count(mp, name, calls):
    fn = getattr(ops._C, name)
    mp.setattr(ops._C, name, lambda *a: calls.append(fn(*a)) or calls[-1])


def _run(mp, x0, x, vw, uw, bias, g, loss=None):
    """The nine results from the public op and autograd; ``loss(y)``
    replaces the backward from ``g``."""
    leaves = [a.cuda().requires_grad_() for a in (x0, x, vw, uw, bias)]
    assert ops.cross_layer_lowrank_kernel_ok(*leaves)
    bwd = []
    _count(mp, "cross_lowrank_bwd_dx", bwd)
    y = ops.cross_layer_lowrank(*leaves)
    t, v = y.grad_fn.saved_tensors[4:6]
    if loss is None:
        grads = torch.autograd.grad(y, leaves, g.cuda())
    else:
        grads = torch.autograd.grad(loss(y), leaves)
    dx0, dx, dv, du, dbias = grads
    (_, dt), = bwd
    return [a.detach().cpu()
            for a in (y, t, v, dx0, dt, dx, du, dv, dbias)]


def _assert_exact(got, want):
    for name, a, r in zip(R.NAMES, got, want):
        w = exact_ints.rne_bf16(r)
        assert a.dtype == BF16 and torch.equal(a, w), name


@pytest.mark.parametrize("b", [1, 129, 300])
@pytest.mark.parametrize("r", [16, 48, 64, 128])
@pytest.mark.parametrize("d", [16, 48, 144, 528])
def test_exact(monkeypatch, d, r, b):
    ops_ = [a.to(BF16) for a in R.int_operands(b, d, r, seed=b + d + r)]
    _assert_exact(_run(monkeypatch, *ops_), R.ref64(*ops_))


@pytest.mark.parametrize("b,d,r,amax,wmax", [(129, 48, 16, 16, 4),
                                             (300, 144, 48, 8, 2)])
def test_exact_rounds(monkeypatch, b, d, r, amax, wmax):
    """Sees a second rounding of ``t``, ``dt``, ``dx``; ``y`` from ``v``."""
    ops_ = [a.to(BF16)
            for a in R.int_operands(b, d, r, seed=1, amax=amax, wmax=wmax)]
    ref = R.ref64(*ops_)
    for name in ("t", "y", "dt", "dx"):
        a = ref[R.NAMES.index(name)]
        err = (exact_ints.rne_bf16(a).double() - a).abs()
        assert (err != 0).any(), f"{name}: nothing to round"
        assert ((err != 0) & (err == exact_ints.bf16_half_ulp(a))).any(), \
            f"{name}: no tie"
    _assert_exact(_run(monkeypatch, *ops_), ref)


def _assert_bounded(operands, got, names=R.NAMES):
    """One bf16 rounding plus the fp32 error of a length-``k`` sum."""
    (b, d), r = operands[1].shape, operands[2].shape[0]
    own = dict(t=got[1], v=got[2], dt=got[4])
    want = R.ref64(*operands, **own)
    mags = R.ref64(*(a.abs() for a in operands),
                   **{k: a.abs() for k, a in own.items()})
    for name, a, w, mag, k in zip(R.NAMES, got, want, mags,
                                  (r, d, r, 1, d, r, b, b, b)):
        if name in names:
            err = (a.double() - w).abs()
            bound = exact_ints.bf16_half_ulp(w) + (k + 2) * 2.0 ** -23 * mag
            print(f"{name}: max err / bound = "
                  f"{(err / bound.clamp_min(1e-300)).max():.3f}")
            assert (err <= bound).all(), name


@pytest.mark.parametrize("b,d,r", [(257, 432, 112), (9, 528, 128)])
def test_bounded(monkeypatch, b, d, r):
    gen = torch.Generator().manual_seed(1)
    x0, x, g = (torch.randn(b, d, generator=gen).to(BF16) for _ in range(3))
    vw = (torch.randn(r, d, generator=gen) * d ** -0.5).to(BF16)
    uw = (torch.randn(d, r, generator=gen) * r ** -0.5).to(BF16)
    bias = torch.randn(d, generator=gen).to(BF16)
    operands = (x0, x, vw, uw, bias, g)
    _assert_bounded(operands, _run(monkeypatch, *operands))


def test_three_row_pitches_give_the_same_bits(monkeypatch):
    b, d, r = 9, 48, 16
    ops_ = [a.to(BF16) for a in R.int_operands(b, d, r, seed=6)]
    x0, x, vw, uw, bias, g = ops_
    want = _run(monkeypatch, *ops_)
    _assert_exact(want, R.ref64(*ops_))
    views = [pitched(a.cuda(), d + extra)
             for a, extra in ((x0, 8), (x, 16), (g, 24))]
    got = _run(monkeypatch, views[0], views[1], vw, uw, bias, views[2])
    for name, a, c in zip(R.NAMES, got, want):
        assert torch.equal(a, c), name


@pytest.mark.parametrize("case", ["sum_over_batch", "sum_of_all"])
def test_grad_y_from_autograd(monkeypatch, case):
    """A ``grad_y`` with row stride 0: the op copies it."""
    b, d, r = 9, 48, 16
    ops_ = [a.to(BF16) for a in R.int_operands(b, d, r, seed=8)]
    g = ops_[5]
    if case == "sum_over_batch":
        g = g[:1].expand(b, -1)
        loss = lambda y: (y.sum(0) * g[0].cuda()).sum()  # noqa: E731
    else:
        g = torch.ones_like(g)
        loss = lambda y: y.sum()  # noqa: E731
    _assert_exact(_run(monkeypatch, *ops_[:5], g, loss),
                  R.ref64(*ops_[:5], g))


def test_empty_batch():
    d, r = 48, 16
    leaves = [torch.ones(s, dtype=BF16, device="cuda", requires_grad=True)
              for s in ((0, d), (0, d), (r, d), (d, r), (d,))]
    assert ops.cross_layer_lowrank_kernel_ok(*leaves)
    y = ops.cross_layer_lowrank(*leaves)
    grads = torch.autograd.grad(y, leaves, torch.zeros_like(y))
    assert [a.shape for a in grads] == [a.shape for a in leaves]
    assert not any(a.any() for a in grads[2:])


def test_no_grad_saves_no_t_or_v(monkeypatch):
    ops_ = [a.to(BF16).cuda() for a in R.int_operands(129, 144, 48, seed=3)]
    ops_[2].requires_grad_()
    results = []
    _count(monkeypatch, "cross_lowrank_fwd", results)
    y_train = ops.cross_layer_lowrank(*ops_[:5])
    with torch.no_grad():
        y_eval = ops.cross_layer_lowrank(*ops_[:5])
    (_, t_train, v_train), (_, t_eval, v_eval) = results
    assert t_train is not None and v_train is not None
    assert t_eval is None and v_eval is None and torch.equal(y_train, y_eval)


SIZES = [7, 5, 3]


def _dcn_step(mp, **kw):
    """One bf16 step of a small DCN; the hook records the second layer."""
    torch.manual_seed(0)
    m = DCN(table_sizes=SIZES, embedding_dim=16, n_cross=3, deep=(32, 16),
            compute_dtype=BF16, **kw).cuda()
    gen = torch.Generator().manual_seed(2)
    dense = torch.randn(8, m.dense_dim, generator=gen).cuda()
    labels = torch.tensor([0., 1., 1., 0.] * 2).cuda()
    ids = torch.tensor([[0, 1, 2], [6, 4, 0], [3, 3, 1], [0, 0, 2]] * 2)
    touched = (ids + m.embedding.offsets.cpu()).reshape(-1)
    seen = []
    m.cross.layers[1].register_forward_hook(  # saved tensors: t and v
        lambda mod, args, out: seen.append(
            (*args, out, *(out.grad_fn.saved_tensors[4:6]
                           if "cross_rank" in kw else ()))))
    calls = {n: [] for n in ("cross_fwd", "cross_lowrank_fwd",
                             "cross_lowrank_bwd_dx")}
    for n, c in calls.items():
        _count(mp, n, c)
    before = m.embedding.weight.detach().cpu()
    loss = m(dense, ids.cuda(), labels)
    loss.backward()
    assert torch.isfinite(loss).item()
    m.apply_sparse_updates(0.1)
    return m, seen, {n: len(c) for n, c in calls.items()}, before, touched


def test_dcn_step_runs_the_kernel_on_its_own_tensors(monkeypatch):
    m, seen, n_calls, before, touched = _dcn_step(monkeypatch, cross_rank=16)
    assert n_calls == {"cross_fwd": 0, "cross_lowrank_fwd": 3,
                       "cross_lowrank_bwd_dx": 3}
    (x0, x, y, t, v), = seen
    la = m.cross.layers[1]
    assert x0.shape == (8, 64) and x.abs().sum() > 0
    operands = [a.detach().cpu() for a in (x0, x, la.v_weight, la.u_weight,
                                           la.bias, torch.zeros(8, 64))]
    got = [y.detach().cpu(), t.cpu(), v.cpu()] + [torch.zeros(1)] * 6
    got[4] = torch.zeros(8, 16)  # dt of the zero grad_y
    _assert_bounded(operands, got, names=("y", "t", "v"))
    for p in la.parameters():
        assert p.grad is not None and p.grad.abs().sum() > 0
    after = m.embedding.weight.detach().cpu()
    is_touched = torch.zeros(sum(SIZES), dtype=torch.bool)
    is_touched[touched] = True
    assert not is_touched.all() and (after != before).any()
    assert torch.equal(after[~is_touched], before[~is_touched])


def test_dcn_switched_off_calls_no_binding(monkeypatch):
    monkeypatch.setenv("MIYARN_CROSS_LAYER", "0")
    assert set(_dcn_step(monkeypatch, cross_rank=16)[2].values()) == {0}


def test_dcn_without_cross_rank_is_full_rank(monkeypatch):
    assert _dcn_step(monkeypatch)[2] == {
        "cross_fwd": 3, "cross_lowrank_fwd": 0, "cross_lowrank_bwd_dx": 0}
