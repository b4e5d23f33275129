"""``ops.cross_layer``'s torch composition against the float64 definition
on integer operands (exact in fp32: see ``cross_layer_ref``), its routing
off the GPU, and ``DCN`` steps on the CPU."""

import pytest
import torch

import cross_layer_ref as R
from tf_yarn_amd import ops
from tf_yarn_amd.models import DCN


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("b,d,amax", [(5, 48, 2), (129, 48, 16),
                                      (300, 144, 16)])
def test_composition_matches_definition(b, d, amax, dtype):
    x0, x, w, bias, g = (t.to(dtype)
                         for t in R.int_operands(b, d, seed=1, amax=amax))
    # autograd keeps v in fp32: dx0's reference is g * v32
    ref = R.ref64(x0, x, w, bias, g, v=R.ref64(x0, x, w, bias, g)[1])
    want = [t.float().to(dtype) for t in ref]
    leaves = [t.requires_grad_() for t in (x0, x, w, bias)]
    assert not ops.cross_layer_kernel_ok(*leaves)
    y = ops.cross_layer(*leaves)
    dx0, dx, dw, dbias = torch.autograd.grad(y, leaves, g)
    assert torch.equal(y, ops._cross_layer_ref(*leaves))
    for name, a, r in zip(("y", "dx0", "dx", "dW", "dbias"),
                          (y, dx0, dx, dw, dbias),
                          (want[0], *want[2:])):
        assert a.dtype == dtype and torch.equal(a, r), name


SIZES = [7, 5, 3]


@pytest.mark.parametrize("multi_hot", [False, True])
def test_dcn_step(multi_hot):
    torch.manual_seed(0)
    kw = dict(table_sizes=SIZES, embedding_dim=16, n_cross=2, deep=(8,))
    m = DCN(**kw)
    b = 4
    dense = torch.randn(b, m.dense_dim)
    labels = torch.tensor([0., 1., 1., 0.])
    offs = m.embedding.offsets
    if multi_hot:
        lens = torch.tensor([1, 2, 0, 3, 1, 1, 2, 2, 1, 0, 1, 2])
        bag_offsets = torch.cat([lens.new_zeros(1), lens.cumsum(0)])
        feat = torch.repeat_interleave(torch.arange(b * 3) % 3, lens)
        ids = torch.tensor([3, 1, 4, 0, 1, 6, 2, 2, 6, 2, 1, 0, 1, 4, 0, 2])
        flat = ids + offs[feat]
        e = torch.nn.functional.embedding_bag(
            flat, m.embedding.weight, bag_offsets[:-1], mode="sum")
    else:
        bag_offsets = None
        ids = torch.tensor([[0, 1, 2], [6, 4, 0], [3, 3, 1], [0, 0, 2]])
        flat = (ids + offs).reshape(-1)
        e = m.embedding.weight[flat]
    # plain torch from the same parameters
    x0 = torch.cat([torch.nn.functional.pad(dense, (0, 16 - m.dense_dim)),
                    e.reshape(b, -1)], dim=1)
    x = x0
    for layer in m.cross.layers:
        x = x0 * (x @ layer.weight.t() + layer.bias) + x
    for layer in m.mlp:
        x = torch.relu(x @ layer.weight.t() + layer.bias)
    want = x @ m.head.weight + m.head.bias
    logits = m(dense, ids, bag_offsets=bag_offsets)
    torch.testing.assert_close(logits, want, rtol=1e-5, atol=1e-6)

    before = m.embedding.weight.detach().clone()
    m(dense, ids, labels, bag_offsets=bag_offsets).backward()
    m.apply_sparse_updates(0.1)
    after = m.embedding.weight.detach()
    untouched = torch.ones(sum(SIZES), dtype=torch.bool)
    untouched[flat] = False
    assert untouched.any() and (after != before).any()
    assert torch.equal(after[untouched], before[untouched])
    assert all(p.grad is not None for p in m.cross.parameters())

    assert sorted(m.state_dict()) == sorted(
        ["embedding.weight", "embedding.offsets",
         "cross.layers.0.weight", "cross.layers.0.bias",
         "cross.layers.1.weight", "cross.layers.1.bias",
         "mlp.0.weight", "mlp.0.bias", "head.weight", "head.bias"])
    m2 = DCN(**kw)
    m2.load_state_dict(m.state_dict())
    assert torch.equal(m2(dense, ids, bag_offsets=bag_offsets),
                       m(dense, ids, bag_offsets=bag_offsets))
