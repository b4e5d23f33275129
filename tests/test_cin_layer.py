"""``ops.cin_layer``'s torch composition against the float64 definition, its
routing off the GPU, and ``XDeepFM`` steps on the CPU."""

import pytest
import torch

import cin_layer_ref as R
from tf_yarn_amd import ops
from tf_yarn_amd.models import CIN, XDeepFM

BF16 = torch.bfloat16


def _run(x0, x, w, g, m):
    assert not ops.cin_layer_kernel_ok(x0.to(BF16), x.to(BF16), w.to(BF16), m)
    return R.run(ops, x0, x, w, g, m)


@pytest.mark.parametrize("amax", [2, 31])
@pytest.mark.parametrize("m,h_in,h_out,d", R.SMALL)
def test_composition_exact(m, h_in, h_out, d, amax):
    first = (m, h_in) == (27, 27) and amax == 2
    x0, x, w, g, r = R.ints(5, m, h_in, h_out, d, amax, first, seed=m)
    R.assert_exact(_run(x0, x, w, g, m), r, first)


@pytest.mark.parametrize("m,h_in,h_out,d", R.SMALL)
def test_composition_bounded(m, h_in, h_out, d):
    x0, x, w, g = R.normal(5, m, h_in, h_out, d)
    r = R.ref64(x0, x, w, g)
    for name, a, want, bound in zip(R.NAMES, _run(x0, x, w, g, m),
                                    r.results, R.bounds(r)):
        assert ((a.double() - want).abs() <= bound).all(), name


@pytest.mark.parametrize("m,h_in,h_out,d", [(4, 3, 16, 24), (33, 2, 16, 16),
                                            (4, 3, 20, 16)])
def test_refused_shapes_take_the_composition(m, h_in, h_out, d):
    x0, x, w, g = R.normal(3, m, h_in, h_out, d)
    assert not ops.cin_layer_kernel_ok(x0, x, w, m)
    y = ops.cin_layer(x0, x, w, m)
    assert y.shape == (3, h_out * d) and y.dtype == BF16
    assert torch.equal(y, ops._cin_layer_ref(x0, x, w, m))
    with pytest.raises(ValueError):
        ops.cin_layer(x0, x[:, 1:], w, m)


def test_fp32_composition_rounds_nothing():
    x0, x, w, g = (t.float() for t in R.normal(3, 4, 3, 16, 16))
    y = ops.cin_layer(x0, x, w, 4)
    want = torch.einsum("hij,bic,bjc->bhc", w.double(),
                        x.double().view(3, 3, 16), x0.double().view(3, 4, 16))
    assert y.dtype == torch.float32
    torch.testing.assert_close(y.double().view(3, 16, 16), want,
                               rtol=1e-5, atol=1e-5)


SIZES = [7, 5, 3]


@pytest.mark.parametrize("multi_hot", [False, True])
def test_xdeepfm_steps(multi_hot):
    torch.manual_seed(0)
    kw = dict(table_sizes=SIZES, embedding_dim=16, bottom=(8,),
              cin=(16, 16), deep=(8,))
    m = XDeepFM(**kw)
    assert isinstance(m.cin, CIN) and m.n_fields == 4
    dense = torch.randn(4, m.dense_dim)
    labels = torch.tensor([0., 1., 1., 0.])
    if multi_hot:
        lens = torch.tensor([1, 2, 0, 3, 1, 1, 2, 2, 1, 0, 1, 2])
        bags = torch.cat([lens.new_zeros(1), lens.cumsum(0)])
        ids = torch.tensor([3, 1, 4, 0, 1, 6, 2, 2, 6, 2, 1, 0, 1, 4, 0, 2])
    else:
        bags = None
        ids = torch.tensor([[0, 1, 2], [6, 4, 0], [3, 3, 1], [0, 0, 2]])
    opt = torch.optim.SGD([p for p in m.parameters()
                           if not getattr(p, "_miyarn_sparse", False)], 0.1)
    losses = []
    for _ in range(4):
        opt.zero_grad()
        loss = m(dense, ids, labels, bag_offsets=bags)
        loss.backward()
        opt.step()
        m.apply_sparse_updates(0.1)
        losses.append(loss.item())
    assert losses[-1] < losses[0]
    assert all(p.grad is not None for p in m.cin.parameters())
    m2 = XDeepFM(**kw)
    m2.load_state_dict(m.state_dict())
    assert torch.equal(m2(dense, ids, bag_offsets=bags),
                       m(dense, ids, bag_offsets=bags))
