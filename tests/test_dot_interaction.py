"""``ops.dot_interaction``'s torch composition against the float64
definition on integer operands (exact in fp32 and bf16: see
``exact_ints``), and ``DLRM`` against a plain-torch model built from the
same parameters."""

import pytest
import torch
import torch.nn.functional as F

import dot_interaction_ref as R
from tf_yarn_amd import ops
from tf_yarn_amd.models import DLRM


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("n,d", [(2, 16), (27, 16), (5, 128), (33, 8)])
def test_composition_matches_definition(n, d, dtype):
    dv, emb, g = (t.to(dtype) for t in R.int_operands(3, n, d))
    want = [t.float().to(dtype) for t in R.ref64(dv, emb, g)]
    dv.requires_grad_()
    emb.requires_grad_()
    out = ops.dot_interaction(dv, emb)
    got = [out, *torch.autograd.grad(out, (dv, emb), g)]
    for a, b in zip(got, want):
        assert a.dtype == dtype and torch.equal(a, b)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("n,d", [(27, 16), (32, 48)])
def test_composition_rounds_like_the_definition(n, d, dtype):
    """Operands in [-16, 16]: fp32 is still exact in any order, and a
    quarter to a half of the values need a real rounding to bf16."""
    dv, emb, g = (t.to(dtype) for t in R.int_operands(3, n, d, seed=1,
                                                      amax=16))
    ref = R.ref64(dv, emb, g)
    want = [t.float().to(dtype) for t in ref]
    if dtype == torch.bfloat16:
        assert all((w.double() != r).any() for w, r in zip(want, ref))
    dv.requires_grad_()
    emb.requires_grad_()
    out = ops.dot_interaction(dv, emb)
    got = [out, *torch.autograd.grad(out, (dv, emb), g)]
    for a, b in zip(got, want):
        assert a.dtype == dtype and torch.equal(a, b)


def _composition(dv, emb, g):
    dv = dv.clone().requires_grad_()
    emb = emb.clone().requires_grad_()
    out = ops.dot_interaction(dv, emb)
    return [out.detach(), *torch.autograd.grad(out, (dv, emb), g)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("where", ["emb", "grad_out"])
def test_composition_keeps_non_finite_values_in_their_example(where, dtype):
    """One +Inf and one NaN in ``emb[1]``, or Infs and a NaN in
    ``grad_out[1]``.  Every other example is bit-identical to the clean
    run, and the forward equals the definition, NaN for NaN.

    The backward of the poisoned example equals the definition when the
    poison is in ``grad_out``.  With the poison in ``emb`` it does NOT: the
    definition sums ``S[i][k] * T[k][c]`` over k, so a non-finite
    ``T[k][c]`` gives NaN where ``S[i][k] == 0`` (the diagonal included) and
    a signed Inf elsewhere.  Autograd's backward of ``bmm`` plus triangle
    gather computes ``L @ T + L^T @ T`` with ``L`` the strictly lower
    triangle of ``S``, so every row i meets the structural zero ``L[i][k]``
    or ``L^T[i][k]`` of every k: a column c of ``T`` that holds a
    non-finite value is NaN in EVERY row of both gradients, where the
    definition (and the HIP kernel) has Infs too.  Columns without poison
    equal the definition bit for bit.  That is what is asserted."""
    n, d, b = 27, 16, 9
    dv, emb, g = (t.to(dtype) for t in R.int_operands(b, n, d, seed=5))
    clean = _composition(dv, emb, g)
    if where == "emb":
        emb = R.poison_emb(emb, d)
    else:
        g = R.poison_grad(g, d)
    want = [t.float().to(dtype) for t in R.ref64(dv, emb, g)]
    got = _composition(dv, emb, g)
    others = [i for i in range(b) if i != 1]
    for a, c, w in zip(got, clean, want):
        assert torch.equal(a[others], c[others])
        assert torch.equal(a[others], w[others])
    assert R.same_bits(got[0], want[0])
    assert not want[1][1].isfinite().all() and not want[2][1].isfinite().all()
    if where == "grad_out":
        assert R.same_bits(got[1], want[1]) and R.same_bits(got[2], want[2])
        return
    t1 = torch.cat([dv[1:2], emb[1].reshape(n - 1, d)])
    bad = ~t1.isfinite().all(0)  # the columns of T that hold the poison
    assert bad.sum() == 2
    dt_got = torch.cat([got[1][1:2], got[2][1].reshape(n - 1, d)])
    dt_want = torch.cat([want[1][1:2], want[2][1].reshape(n - 1, d)])
    assert torch.equal(dt_got[:, ~bad], dt_want[:, ~bad])
    assert dt_got[:, bad].isnan().all()
    assert dt_want[:, bad].isinf().any()  # the difference is real


def test_width():
    assert ops.dot_interaction_width(26, 16) == 368
    assert ops.dot_interaction_width(1, 16) == 32


def _plain_logits(m, table, dense, flat_ids, bag_offsets):
    """DLRM's forward in plain torch from ``m``'s dense parameters and
    ``table``; ``flat_ids`` already carry the table offsets."""
    x = F.pad(dense, (0, m.dense_pad))
    for layer in m.bottom_mlp:
        x = torch.relu(x @ layer.weight.t() + layer.bias)
    b, d = x.shape
    if bag_offsets is None:
        e = F.embedding(flat_ids, table)
    else:
        e = F.embedding_bag(flat_ids, table, bag_offsets[:-1], mode="sum")
    t = torch.cat([x, e.reshape(b, -1)], dim=1).reshape(b, -1, d)
    n = t.shape[1]
    i, j = torch.tril_indices(n, n, offset=-1)
    pairs = torch.bmm(t, t.transpose(1, 2))[:, i, j]
    z = F.pad(torch.cat([x, pairs], dim=1),
              (0, m.top_mlp[0].weight.shape[1] - d - i.numel()))
    for layer in m.top_mlp:
        z = torch.relu(z @ layer.weight.t() + layer.bias)
    return z @ m.head.weight + m.head.bias


@pytest.mark.parametrize("multi_hot", [False, True])
def test_dlrm_matches_plain_torch(multi_hot):
    torch.manual_seed(0)
    sizes = [7, 5, 3]
    kw = dict(table_sizes=sizes, embedding_dim=16, bottom=(8,), top=(8,))
    m = DLRM(**kw)
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
    else:
        bag_offsets = None
        ids = torch.tensor([[0, 1, 2], [6, 4, 0], [3, 3, 1], [0, 0, 2]])
        flat = ids + offs
    before = m.embedding.weight.detach().clone()
    table = before.clone().requires_grad_()
    want = _plain_logits(m, table, dense, flat, bag_offsets)
    F.binary_cross_entropy_with_logits(want, labels).backward()

    logits = m(dense, ids, bag_offsets=bag_offsets)
    torch.testing.assert_close(logits, want, rtol=1e-6, atol=2 ** -23)
    m(dense, ids, labels, bag_offsets=bag_offsets).backward()
    m.apply_sparse_updates(0.1)
    after = m.embedding.weight.detach()
    # atol: one fp32 ulp at the magnitude of the largest table values
    torch.testing.assert_close(after, before - 0.1 * table.grad, rtol=1e-6,
                               atol=2 ** -23)
    untouched = torch.ones(sum(sizes), dtype=torch.bool)
    untouched[flat.reshape(-1)] = False
    assert untouched.any() and (after != before).any()
    assert torch.equal(after[untouched], before[untouched])

    m2 = DLRM(**kw)
    m2.load_state_dict(m.state_dict())
    assert torch.equal(m2(dense, ids, bag_offsets=bag_offsets),
                       m(dense, ids, bag_offsets=bag_offsets))
