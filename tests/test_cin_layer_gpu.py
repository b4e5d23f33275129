"""The CIN-layer HIP kernels (``csrc/cin_layer.hip``) against the float64
definition, through the public op and autograd.  The integer cases
(``cin_layer_ref.ints``) must give ``rne_bf16`` of the float64 results bit
for bit.  ``B = 21`` on one block makes two trips, the second with idle
waves; ``B = 37`` on two splits the weight gradient's k-steps 10 : 9, the
last one half full."""

import pytest
import torch

import cin_layer_ref as R
from dot_interaction_ref import pitched, same_bits
from tf_yarn_amd import ops
from tf_yarn_amd.models import XDeepFM

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X"),
]

BF16 = torch.bfloat16
BATCHES = [(1, None), (5, None), (21, 1), (37, 2)]  # (B, max_blocks)


def _run(x0, x, w, g, m, max_blocks=None, loss=None):
    first = x is x0
    x0, x, w, g = (t.to(device="cuda", dtype=BF16) for t in (x0, x, w, g))
    x = x0 if first else x
    assert ops.cin_layer_kernel_ok(x0, x, w, m)
    return R.run(ops, x0, x, w, g, m, max_blocks, loss, device="cuda")


@pytest.mark.parametrize("b,max_blocks", BATCHES)
@pytest.mark.parametrize("m,h_in,h_out,d", R.SHAPES)
def test_small_ints(m, h_in, h_out, d, b, max_blocks):
    first = (m, h_in) == (27, 27)  # the Criteo first layer: x is x0
    x0, x, w, g, r = R.ints(b, m, h_in, h_out, d, first=first, seed=m + b)
    R.assert_exact(_run(x0, x, w, g, m, max_blocks), r, first)


@pytest.mark.parametrize("b,max_blocks", BATCHES[1:3])
@pytest.mark.parametrize("m,h_in,h_out,d", R.SMALL)
def test_rounded_z(m, h_in, h_out, d, b, max_blocks):
    x0, x, w, g, r = R.ints(b, m, h_in, h_out, d, amax=31, seed=m + b)
    R.assert_exact(_run(x0, x, w, g, m, max_blocks), r)


@pytest.mark.parametrize("b,m,h_in,h_out,d",
                         [(67, 27, 27, 32, 16), (37, 32, 40, 64, 32)])
def test_bounded(b, m, h_in, h_out, d):
    x0, x, w, g = R.normal(b, m, h_in, h_out, d)
    r = R.ref64(x0, x, w, g)
    got = _run(x0, x, w, g, m, max_blocks=2)
    for name, a, want, bound in zip(R.NAMES, got, r.results, R.bounds(r)):
        err = (a.double() - want).abs()
        print(f"{name}: max err / bound = "
              f"{(err / bound.clamp_min(1e-300)).max():.3f}")
        assert (err <= bound).all(), name
    again = _run(x0, x, w, g, m, max_blocks=2)
    assert torch.equal(again[3], got[3]), "dW is not deterministic"


def test_row_pitches_give_the_same_bits():
    """``x0``, ``x`` and ``grad_y`` in buffers 8 and 16 columns wider, the
    gaps full of NaN."""
    b, m, h_in, h_out, d = 5, 27, 32, 48, 16
    x0, x, w, g = R.normal(b, m, h_in, h_out, d)
    want = _run(x0, x, w, g, m)
    views = [pitched(t.cuda(), t.shape[1] + pad)
             for t, pad in ((x0, 8), (x, 16), (g, 8))]
    assert ops._C.cin_layer_rows_ok(views[2])
    got = _run(views[0], views[1], w, views[2], m)
    for a, c in zip(got, want):
        assert torch.equal(a, c)


def test_pooled_loss_hands_over_a_broadcast_gradient():
    """Row and column stride 0, which the bindings refuse: the op copies."""
    b, m, h_in, h_out, d = 5, 5, 5, 16, 16
    x0, x, w, g, _ = R.ints(b, m, h_in, h_out, d, seed=3)
    g = torch.ones_like(g)
    loss = lambda y: y.view(b, h_out, d).float().sum(-1).sum()  # noqa: E731
    R.assert_exact(_run(x0, x, w, g, m, loss=loss), R.ref64(x0, x, w, g))


def test_empty_batch():
    x0 = torch.zeros(0, 27 * 16, dtype=BF16, device="cuda",
                     requires_grad=True)
    w = torch.ones(32, 27, 27, dtype=BF16, device="cuda", requires_grad=True)
    assert ops.cin_layer_kernel_ok(x0, x0, w, 27)
    y = ops.cin_layer(x0, x0, w, 27)
    dx0, dw = torch.autograd.grad(y, (x0, w), torch.zeros_like(y))
    torch.cuda.synchronize()
    assert y.shape == (0, 32 * 16) and y.dtype == BF16
    assert dx0.shape == x0.shape and dw.shape == w.shape and not dw.any()


def test_non_finite_values_stay_in_their_example():
    b, m, h_in, h_out, d = 9, 5, 6, 16, 16
    x0, x, w, g = R.normal(b, m, h_in, h_out, d)
    clean = _run(x0, x, w, g, m, max_blocks=1)
    bad0, bad = x0.clone(), x.clone()
    bad0[4, 2 * d + 5] = float("inf")
    bad[4, 3 * d + 1] = float("nan")
    got = _run(bad0, bad, w, g, m, max_blocks=1)
    keep = torch.arange(b) != 4
    for name, a, c in list(zip(R.NAMES, got, clean))[:3]:
        assert same_bits(a[keep], c[keep]) and a[keep].isfinite().all(), name


# ---- XDeepFM on the GPU ----------------------------------------------------

SIZES = [7, 5, 3]
CALLS = ("cin_layer_fwd", "cin_layer_bwd_data", "cin_layer_bwd_weight")


def _xdeepfm_step(monkeypatch, multi_hot=False, dtype=BF16):
    """One training step of a small XDeepFM: the binding calls, the table
    before and after, the touched rows."""
    torch.manual_seed(0)
    model = XDeepFM(table_sizes=SIZES, embedding_dim=16, bottom=(32,),
                    cin=(16, 16), deep=(16,), compute_dtype=dtype).cuda()
    gen = torch.Generator().manual_seed(2)
    dense = torch.randn(8, model.dense_dim, generator=gen).cuda()
    labels = torch.tensor([0., 1., 1., 0.] * 2).cuda()
    ids = torch.tensor([[0, 1, 2], [6, 4, 0], [3, 3, 1], [0, 0, 2]] * 2)
    field = torch.arange(3).expand(8, 3)
    bags = None
    if multi_hot:  # two ids in every other bag
        lens = torch.tensor([1, 2] * 12)
        bags = torch.cat([lens.new_zeros(1), lens.cumsum(0)]).cuda()
        ids, field = (t.reshape(-1).repeat_interleave(lens)
                      for t in (ids, field))
    touched = ids.reshape(-1) + model.embedding.offsets.cpu()[
        field.reshape(-1)]
    calls = dict.fromkeys(CALLS, 0)
    for name in CALLS:
        def counted(*a, _f=getattr(ops._C, name), _n=name):
            calls[_n] += 1
            return _f(*a)
        monkeypatch.setattr(ops._C, name, counted)
    before = model.embedding.weight.detach().cpu()
    loss = model(dense, ids.cuda(), labels, bag_offsets=bags)
    loss.backward()
    assert torch.isfinite(loss).item()
    assert all(p.grad is not None and p.grad.abs().sum() > 0
               for p in model.cin.parameters())
    model.apply_sparse_updates(0.1)
    return calls, before, model.embedding.weight.detach().cpu(), touched


@pytest.mark.parametrize("multi_hot", [False, True])
def test_xdeepfm_step_runs_the_kernels(monkeypatch, multi_hot):
    calls, before, after, touched = _xdeepfm_step(monkeypatch, multi_hot)
    assert calls == dict.fromkeys(CALLS, 2)
    is_touched = torch.zeros(sum(SIZES), dtype=torch.bool)
    is_touched[touched] = True
    assert not is_touched.all() and (after != before).any()
    assert torch.equal(after[~is_touched], before[~is_touched])


@pytest.mark.parametrize("how", ["switched_off", "fp32"])
def test_xdeepfm_without_the_kernels_calls_no_binding(monkeypatch, how):
    if how == "switched_off":
        monkeypatch.setenv("MIYARN_CIN_LAYER", "0")
    calls = _xdeepfm_step(
        monkeypatch, dtype=BF16 if how == "switched_off" else torch.float32)[0]
    assert calls == dict.fromkeys(CALLS, 0)
