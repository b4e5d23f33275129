"""``ops.field_attention``'s torch composition against the float64
definition, its routing off the GPU, and ``AutoInt`` steps on the CPU."""

import pytest
import torch

import exact_ints
import field_attention_ref as R
from tf_yarn_amd import ops
from tf_yarn_amd.models import AutoInt

BF16 = torch.bfloat16


def _run(qkv, g, n, h, scale):
    qkv = qkv.to(BF16).requires_grad_()
    assert not ops.field_attention_kernel_ok(qkv, n, h)
    out = ops.field_attention(qkv, n, h, scale)
    dqkv, = torch.autograd.grad(out, qkv, g.to(BF16))
    return (out.detach(), *dqkv.chunk(3, dim=1))


@pytest.mark.parametrize("case", ["selective", "uniform_q", "uniform_k"])
def test_composition_exact(case):
    if case == "selective":
        qkv, g, scale, r = R.selective(3, 5, 2, 16, seed=1)
        n, h = 5, 2
    else:
        qkv, g, scale, r = R.uniform(3, 8, 4, 16, case[-1], seed=2)
        n, h = 8, 4
    for name, a, want in zip(R.NAMES, _run(qkv, g, n, h, scale), r.results):
        assert torch.equal(a, exact_ints.rne_bf16(want)), name


def test_composition_bounded():
    n, h, d = 27, 2, 16
    qkv, g, scale = R.normal(5, n, h, d)
    r = R.ref64(qkv, g, n, h, scale)
    for name, a, want, bound in zip(R.NAMES, _run(qkv, g, n, h, scale),
                                    r.results, R.bounds(r, n, d)):
        assert ((a.double() - want).abs() <= bound).all(), name


@pytest.mark.parametrize("n,h,d", [(33, 1, 16), (4, 1, 8), (4, 5, 64),
                                   (4, 1, 48)])
def test_refused_shapes_take_the_composition(n, h, d):
    qkv = torch.randn(2 * n, 3 * h * d).to(BF16)
    assert not ops.field_attention_kernel_ok(qkv, n, h)
    assert not ops.field_attention_kernel_ok(qkv[:, 1:], n, h)
    out = ops.field_attention(qkv, n, h)
    assert out.shape == (2 * n, h * d) and out.dtype == BF16
    with pytest.raises(ValueError):
        ops.field_attention(qkv[1:], n, h)


SIZES = [7, 5, 3]


@pytest.mark.parametrize("multi_hot", [False, True])
def test_autoint_steps(multi_hot):
    torch.manual_seed(0)
    kw = dict(table_sizes=SIZES, embedding_dim=16, bottom=(8,), n_layers=2,
              n_heads=2, head_dim=16, deep=(8,))
    m = AutoInt(**kw)
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
    assert all(p.grad is not None for p in m.layers.parameters())
    m2 = AutoInt(**kw)
    m2.load_state_dict(m.state_dict())
    assert torch.equal(m2(dense, ids, bag_offsets=bags),
                       m(dense, ids, bag_offsets=bags))
