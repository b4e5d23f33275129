"""The field-attention HIP kernels (``csrc/field_attention.hip``) against the
float64 definition, through the public op and autograd.  The exact cases
(``field_attention_ref``) must give ``rne_bf16`` of the float64 results bit
for bit; ``B = 9`` in one block makes three trips, the last ragged."""

import pytest
import torch

import exact_ints
import field_attention_ref as R
from dot_interaction_ref import pitched, same_bits
from tf_yarn_amd import ops
from tf_yarn_amd.models import AutoInt

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X"),
]

BF16 = torch.bfloat16
SHAPES = [(2, 1, 16), (5, 2, 16), (16, 2, 16), (27, 2, 16), (31, 3, 32),
          (32, 1, 32), (32, 2, 64), (8, 4, 16)]
UNIFORM = [(8, 4, 16), (16, 2, 16), (32, 1, 32), (32, 2, 64)]
BATCHES = [(1, 0), (5, 0), (9, 1)]  # (B, max_blocks)


def _run(qkv, g, n, h, scale, max_blocks=0, loss=None):
    """(out, dQ, dK, dV) on the CPU; ``loss(out)`` replaces ``g``."""
    qkv, g = (t if t.is_cuda else t.to(BF16).cuda() for t in (qkv, g))
    qkv = qkv.detach().requires_grad_()
    assert ops.field_attention_kernel_ok(qkv, n, h)
    out = ops.field_attention(qkv, n, h, scale, max_blocks)
    if loss is None:
        dqkv, = torch.autograd.grad(out, qkv, g)
    else:
        dqkv, = torch.autograd.grad(loss(out), qkv)
    assert dqkv.is_contiguous()
    return [t.detach().cpu() for t in (out, *dqkv.chunk(3, dim=1))]


def _assert_exact(got, r):
    for name, a, want in zip(R.NAMES, got, r.results):
        w = exact_ints.rne_bf16(want)
        assert a.dtype == BF16 and a.shape == w.shape, name
        assert torch.equal(a, w), name


@pytest.mark.parametrize("b,max_blocks", BATCHES)
@pytest.mark.parametrize("n,h,d", SHAPES)
def test_selective(n, h, d, b, max_blocks):
    qkv, g, scale, r = R.selective(b, n, h, d, seed=n + b)
    _assert_exact(_run(qkv, g, n, h, scale, max_blocks), r)


@pytest.mark.parametrize("b,max_blocks", BATCHES)
@pytest.mark.parametrize("zero", ["q", "k"])
@pytest.mark.parametrize("n,h,d", UNIFORM)
def test_uniform(n, h, d, zero, b, max_blocks):
    qkv, g, scale, r = R.uniform(b, n, h, d, zero, seed=n + b)
    _assert_exact(_run(qkv, g, n, h, scale, max_blocks), r)


@pytest.mark.parametrize("b,n,h,d", [(257, 27, 2, 16), (9, 32, 2, 64)])
def test_bounded(b, n, h, d):
    qkv, g, scale = R.normal(b, n, h, d)
    r = R.ref64(qkv, g, n, h, scale)
    got = _run(qkv, g, n, h, scale)
    for name, a, want, bound in zip(R.NAMES, got, r.results,
                                    R.bounds(r, n, d)):
        err = (a.double() - want).abs()
        print(f"{name}: max err / bound = "
              f"{(err / bound.clamp_min(1e-300)).max():.3f}")
        assert (err <= bound).all(), name


def test_row_pitches_give_the_same_bits():
    """``qkv`` and ``grad_out`` in buffers ``H*d`` and 8 columns wider,
    the gaps full of NaN."""
    b, n, h, d = 5, 27, 2, 16
    qkv, g, scale = R.normal(b, n, h, d)
    want = _run(qkv, g, n, h, scale)
    views = [pitched(qkv.cuda(), 4 * h * d), pitched(g.cuda(), h * d + 8)]
    assert [v.stride(0) for v in views] == [4 * h * d, h * d + 8]
    assert ops._C.field_attention_rows_ok(views[1])
    for a, c in zip(_run(*views, n, h, scale), want):
        assert torch.equal(a, c)


@pytest.mark.parametrize("case", ["sum_over_rows", "sum_of_all"])
def test_grad_out_from_autograd(case):
    """Row stride 0, which the binding refuses: the op copies it."""
    b, n, h, d = 5, 5, 2, 16
    qkv, g, scale, _ = R.selective(b, n, h, d, seed=3)
    if case == "sum_over_rows":
        g = g[:1].expand(b * n, -1)
        loss = lambda out: (out.sum(0) * g[0].to(BF16).cuda()).sum()  # noqa
    else:
        g = torch.ones_like(g)
        loss = lambda out: out.sum()  # noqa: E731
    _assert_exact(_run(qkv, g, n, h, scale, loss=loss),
                  R.ref64(qkv, g, n, h, scale))


def test_empty_batch():
    qkv = torch.zeros(0, 96, dtype=BF16, device="cuda", requires_grad=True)
    assert ops.field_attention_kernel_ok(qkv, 27, 2)
    out = ops.field_attention(qkv, 27, 2)
    dqkv, = torch.autograd.grad(out, qkv, torch.zeros_like(out))
    torch.cuda.synchronize()
    assert out.shape == (0, 32) and out.dtype == BF16
    assert dqkv.shape == (0, 96)


def test_non_finite_values_stay_in_their_example():
    b, n, h, d = 9, 16, 2, 16
    qkv, g, scale = R.normal(b, n, h, d)
    clean = _run(qkv, g, n, h, scale, max_blocks=1)
    bad = qkv.clone()
    bad[4 * n + 3, 5] = float("inf")             # a query of example 4
    bad[4 * n + 7, h * d + d + 2] = float("nan")  # a key, head 1
    bad[4 * n + 9, 2 * h * d + 1] = float("inf")  # a value
    got = _run(bad, g, n, h, scale, max_blocks=1)
    keep = torch.ones(b * n, dtype=torch.bool)
    keep[4 * n:5 * n] = False
    for name, a, c in zip(R.NAMES, got, clean):
        assert same_bits(a[keep], c[keep]) and a[keep].isfinite().all(), name


# ---- AutoInt on the GPU ----------------------------------------------------

SIZES = [7, 5, 3]


def _autoint_step(monkeypatch, dtype=BF16):
    """One one-hot training step of a small AutoInt: the binding calls,
    the table before and after, the touched rows."""
    torch.manual_seed(0)
    m = AutoInt(table_sizes=SIZES, embedding_dim=16, bottom=(32,),
                n_layers=3, deep=(16,), compute_dtype=dtype).cuda()
    gen = torch.Generator().manual_seed(2)
    dense = torch.randn(8, m.dense_dim, generator=gen).cuda()
    labels = torch.tensor([0., 1., 1., 0.] * 2).cuda()
    ids = torch.tensor([[0, 1, 2], [6, 4, 0], [3, 3, 1], [0, 0, 2]] * 2)
    touched = (ids + m.embedding.offsets.cpu()).reshape(-1)
    calls = {"field_attention_fwd": 0, "field_attention_bwd": 0}
    for name in calls:
        def counted(*a, _f=getattr(ops._C, name), _n=name):
            calls[_n] += 1
            return _f(*a)
        monkeypatch.setattr(ops._C, name, counted)
    before = m.embedding.weight.detach().cpu()
    loss = m(dense, ids.cuda(), labels)
    loss.backward()
    assert torch.isfinite(loss).item()
    assert all(p.grad is not None and p.grad.abs().sum() > 0
               for p in m.layers.parameters())
    m.apply_sparse_updates(0.1)
    return calls, before, m.embedding.weight.detach().cpu(), touched


def test_autoint_step_runs_the_kernels(monkeypatch):
    calls, before, after, touched = _autoint_step(monkeypatch)
    assert calls == {"field_attention_fwd": 3, "field_attention_bwd": 3}
    is_touched = torch.zeros(sum(SIZES), dtype=torch.bool)
    is_touched[touched] = True
    assert not is_touched.all() and (after != before).any()
    assert torch.equal(after[~is_touched], before[~is_touched])


@pytest.mark.parametrize("how", ["switched_off", "fp32"])
def test_autoint_without_the_kernels_calls_no_binding(monkeypatch, how):
    if how == "switched_off":
        monkeypatch.setenv("MIYARN_FIELD_ATTENTION", "0")
    calls = _autoint_step(
        monkeypatch, BF16 if how == "switched_off" else torch.float32)[0]
    assert calls == {"field_attention_fwd": 0, "field_attention_bwd": 0}
