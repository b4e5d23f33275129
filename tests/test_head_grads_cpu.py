"""CPU references of ``col_reduce_dot_sum`` and ``head_relu_bwd_grads``, and
the autograd nodes with MIYARN_FUSED_HEAD_GRADS on and off: without a GPU
the switch must change nothing."""

import pytest
import torch

from tf_yarn_amd import ops


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_col_reduce_dot_sum_cpu(dtype):
    gen = torch.Generator().manual_seed(3)
    x = torch.randint(-2, 3, (37, 12), generator=gen).to(dtype)
    dy = torch.randint(-2, 3, (37,), generator=gen).to(dtype)
    dw, db = ops.col_reduce_dot_sum(x, dy, dtype)
    assert dw.dtype == dtype and db.dtype == dtype and db.shape == (1,)
    assert torch.equal(dw.double(), dy.double() @ x.double())
    assert torch.equal(db.double(), dy.double().sum().reshape(1))
    assert torch.equal(dw.float(), ops.col_reduce_dot(x, dy))


def test_head_relu_bwd_grads_cpu_is_the_separate_pieces():
    gen = torch.Generator().manual_seed(4)
    dl = torch.randn(21, generator=gen)
    w = torch.randn(16, generator=gen)
    y = torch.relu(torch.randn(21, 16, generator=gen))
    dz, dbias, dw_head, db_head = ops.head_relu_bwd_grads(dl, w, y)
    want_dz, want_db = ops.head_relu_bwd_db(dl, w, y)
    assert torch.equal(dz, want_dz) and torch.equal(dbias, want_db)
    assert torch.equal(dw_head, ops.col_reduce_dot(y, dl))
    assert torch.equal(db_head, dl.sum().reshape(1))


@pytest.mark.parametrize("switch", ["1", "0"])
def test_autograd_nodes_on_cpu(switch, monkeypatch):
    monkeypatch.setenv("MIYARN_FUSED_HEAD_GRADS", switch)
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(21, 8, generator=gen)
    wt = torch.randn(16, 8, generator=gen).requires_grad_()
    bias = torch.randn(16, generator=gen).requires_grad_()
    w_head = torch.randn(16, generator=gen).requires_grad_()
    b_head = torch.randn(1, generator=gen).requires_grad_()
    out = ops.linear_bias_relu_head(x, wt, bias, w_head, b_head)
    ref = torch.relu(x @ wt.detach().t() + bias.detach()) @ w_head.detach() \
        + b_head.detach()
    assert torch.allclose(out, ref, atol=1e-5)
    dl = torch.randn(21, generator=gen)
    out.backward(dl)
    y = torch.relu(x @ wt.detach().t() + bias.detach())
    assert torch.allclose(w_head.grad, dl @ y, atol=1e-5)
    assert torch.allclose(b_head.grad, dl.sum().reshape(1), atol=1e-5)
    w2 = torch.randn(8, generator=gen).requires_grad_()
    b2 = torch.randn(1, generator=gen).requires_grad_()
    ops.ScalarHeadFn.apply(x, w2, b2).backward(dl)
    assert torch.allclose(w2.grad, dl @ x, atol=1e-5)
    assert torch.allclose(b2.grad, dl.sum().reshape(1), atol=1e-5)
