"""``ops.cross_layer_lowrank``'s torch composition against the float64
definition on exact integer operands; ``DCN(cross_rank=...)`` on the CPU."""

import pytest
import torch

import cross_lowrank_ref as R
from tf_yarn_amd import ops
from tf_yarn_amd.models import DCN, LowRankCrossLayer


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("b,d,r,amax,wmax", [(5, 48, 16, 2, 2),
                                             (129, 48, 16, 16, 4),
                                             (300, 144, 48, 8, 2)])
def test_composition_matches_definition(b, d, r, amax, wmax, dtype):
    """Autograd keeps ``v`` in fp32, ``t`` and ``dt`` in ``x``'s dtype."""
    ints = R.int_operands(b, d, r, seed=1, amax=amax, wmax=wmax)
    x0, x, vw, uw, bias, g = (a.to(dtype) for a in ints)
    fp32 = dtype == torch.float32
    first = R.ref64(*ints)
    t = first[1] if fp32 else None
    first = R.ref64(*ints, t=t)
    ref = R.ref64(*ints, t=t, v=first[2], dt=first[4] if fp32 else None)
    leaves = [a.requires_grad_() for a in (x0, x, vw, uw, bias)]
    assert not ops.cross_layer_lowrank_kernel_ok(*leaves)
    y = ops.cross_layer_lowrank(*leaves)
    assert torch.equal(y, ops._cross_layer_lowrank_ref(*leaves))
    dx0, dx, dv, du, dbias = torch.autograd.grad(y, leaves, g)
    for name, a in zip(R.NAMES, (y, None, None, dx0, None, dx, du, dv,
                                 dbias)):
        if a is not None:
            want = ref[R.NAMES.index(name)].float().to(dtype)
            assert a.dtype == dtype and torch.equal(a, want), name


@pytest.mark.parametrize("r,d,dtype", [(24, 48, torch.bfloat16),
                                       (16, 40, torch.bfloat16),
                                       (16, 48, torch.float32)])
def test_refused_shapes_do_not_raise(r, d, dtype):
    gen = torch.Generator().manual_seed(0)
    x0, x = (torch.randn(3, d, generator=gen).to(dtype) for _ in range(2))
    layer = LowRankCrossLayer(d, r, dtype)
    y = layer(x0, x)
    y.float().sum().backward()
    assert all(p.grad is not None for p in layer.parameters())


KW = dict(table_sizes=[7, 5, 3], embedding_dim=16, n_cross=2, deep=(8,))


@pytest.mark.parametrize("multi_hot", [False, True])
def test_dcn_lowrank_step(multi_hot):
    torch.manual_seed(0)
    m = DCN(cross_rank=16, **KW)
    dense = torch.randn(4, m.dense_dim)
    labels = torch.tensor([0., 1., 1., 0.])
    if multi_hot:
        lens = torch.tensor([1, 2, 0, 3, 1, 1, 2, 2, 1, 0, 1, 2])
        bag_offsets = torch.cat([lens.new_zeros(1), lens.cumsum(0)])
        ids = torch.tensor([3, 1, 4, 0, 1, 6, 2, 2, 6, 2, 1, 0, 1, 4, 0, 2])
    else:
        bag_offsets = None
        ids = torch.tensor([[0, 1, 2], [6, 4, 0], [3, 3, 1], [0, 0, 2]])
    before = m.embedding.weight.detach().clone()
    m(dense, ids, labels, bag_offsets=bag_offsets).backward()
    m.apply_sparse_updates(0.1)
    assert (m.embedding.weight != before).any()
    assert all(p.grad is not None and p.grad.abs().sum() > 0
               for p in m.cross.parameters())
    assert [k for k in m.state_dict() if k.startswith("cross.layers.1")] == [
        "cross.layers.1.v_weight", "cross.layers.1.u_weight",
        "cross.layers.1.bias"]


def test_cross_rank_none_is_todays_model():
    torch.manual_seed(3)
    a = DCN(**KW)
    torch.manual_seed(3)
    b = DCN(cross_rank=None, **KW)
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb) and "cross.layers.0.weight" in sa
    assert all(torch.equal(sa[k], sb[k]) for k in sa)
