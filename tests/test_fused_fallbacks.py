"""CPU side of the fused lookup / head-backward work: without a GPU the new
ops ARE the composition of the ops they replace on the GPU, so results on
the CPU cannot move, and the model gives the same two training steps with
the MIYARN_FUSED_LOOKUP / MIYARN_FUSED_HEAD_BWD switches on and off.
"""

import pytest
import torch

from tf_yarn_amd import ops


def _lookup_operands(b, f, dim, n_dense, rpf, seed):
    gen = torch.Generator().manual_seed(seed)
    table = torch.randn(f * rpf, dim, generator=gen)
    wide = torch.randn(f * rpf, 1, generator=gen)
    ids = torch.randint(0, rpf, (b, f), generator=gen)
    offsets = torch.arange(f, dtype=torch.int64) * rpf
    dense = torch.randn(b, n_dense, generator=gen)
    return table, wide, ids, offsets, dense


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16],
                         ids=["f32", "bf16"])
@pytest.mark.parametrize("b,f,dim,n_dense,col_offset",
                         [(5, 26, 16, 13, 16), (1, 1, 4, 0, 0),
                          (7, 3, 7, 1, 2)])
def test_lookup_fused_cpu_is_the_separate_ops(b, f, dim, n_dense,
                                              col_offset, dtype):
    table, wide, ids, offsets, dense = _lookup_operands(
        b, f, dim, n_dense, 9, seed=b + dim)
    dense = dense.to(dtype)
    want = torch.full((b, col_offset + f * dim + 3), 3.0, dtype=dtype)
    got = want.clone()
    assert not ops.emb_lookup_fused_covers(table, ids, dense, got,
                                           col_offset)
    flat = (ids + offsets.unsqueeze(0)).reshape(-1)
    want[:, :n_dense] = dense
    want[:, n_dense:col_offset] = 0
    ops.emb_fwd_into(table, flat, want, col_offset)
    want_wide = ops.emb_gather_sum(wide, flat.reshape(b, f),
                                   dtype == torch.bfloat16)
    got_wide = ops.emb_lookup_fused(table, wide, ids, offsets, dense, got,
                                    col_offset)
    assert got_wide.dtype == want_wide.dtype
    assert torch.equal(got, want)
    assert torch.equal(got_wide, want_wide)


@pytest.mark.parametrize("strided", [False, True], ids=["dense", "slice"])
def test_scatter_offsets_cpu_is_the_pre_added_ids(strided):
    b, f, dim, rpf = 33, 4, 8, 5  # rows repeat: index_add_ order is fixed
    table, wide, ids, offsets, _ = _lookup_operands(b, f, dim, 0, rpf, 1)
    gen = torch.Generator().manual_seed(2)
    grad = torch.randn(b, 16 + f * dim, generator=gen)
    grad = grad[:, 16:] if strided else grad[:, 16:].contiguous()
    gw = torch.randn(b, generator=gen)
    t_raw, w_raw = table.clone(), wide.clone()
    ops.emb_bwd_sgd_fused_wide(t_raw, w_raw, ids, grad, gw, lr=0.3,
                               scale=0.5, offsets=offsets)
    t_flat, w_flat = table.clone(), wide.clone()
    ops.emb_bwd_sgd_fused_wide(
        t_flat, w_flat, (ids + offsets.unsqueeze(0)).reshape(-1), grad, gw,
        lr=0.3, scale=0.5)
    assert not torch.equal(t_raw, table)
    assert torch.equal(t_raw, t_flat)
    assert torch.equal(w_raw, w_flat)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16],
                         ids=["f32", "bf16"])
def test_head_relu_bwd_db_cpu_is_the_two_step_path(dtype):
    gen = torch.Generator().manual_seed(5)
    rows, cols = 19, 24
    dl = torch.randn(rows, generator=gen).to(dtype)
    w = torch.randn(cols, generator=gen).to(dtype)
    y = torch.relu(torch.randn(rows, cols, generator=gen)).to(dtype)
    dz, dbias = ops.head_relu_bwd_db(dl, w, y)
    want = ops.bias_relu_bwd(dl.unsqueeze(1) * w.unsqueeze(0), y)
    assert torch.equal(dz, want)
    assert torch.equal(dbias, want.sum(dim=0))


def test_linear_bias_relu_head_cpu_matches_the_two_modules():
    """One autograd node against FusedLinearReLU followed by ScalarHead:
    output and all five gradients."""
    gen = torch.Generator().manual_seed(6)
    b, k, n = 12, 20, 8
    vals = [torch.randn(b, k, generator=gen), torch.randn(n, k, generator=gen),
            torch.randn(n, generator=gen), torch.randn(n, generator=gen),
            torch.randn(1, generator=gen)]
    g = torch.randn(b, generator=gen)
    results = []
    for fused in (True, False):
        x, w, bias, wh, bh = [v.clone().requires_grad_(True) for v in vals]
        if fused:
            out = ops.linear_bias_relu_head(x, w, bias, wh, bh)
        else:
            out = ops.ScalarHeadFn.apply(ops.linear_bias_relu(x, w, bias),
                                         wh, bh)
        out.backward(g)
        results.append([out.detach()] + [t.grad for t in (x, w, bias, wh, bh)])
    for a, c in zip(*results):
        assert torch.equal(a, c)


def _train_two_steps(monkeypatch, switch):
    from tf_yarn_amd.models.wide_deep import WideAndDeep
    from tf_yarn_amd.ops.optim import FusedSGD
    monkeypatch.setenv("MIYARN_FUSED_LOOKUP", switch)
    monkeypatch.setenv("MIYARN_FUSED_HEAD_BWD", switch)
    f, rpf, b = 6, 40, 32
    torch.manual_seed(3)
    model = WideAndDeep(table_sizes=[rpf] * f, embedding_dim=8,
                        hidden=(16, 8), sharded=True)
    opt = FusedSGD([p for p in model.parameters()
                    if not getattr(p, "_miyarn_sparse", False)], lr=0.05)
    gen = torch.Generator().manual_seed(4)
    losses = []
    for _ in range(2):
        ids = torch.stack([torch.randperm(rpf, generator=gen)[:b]
                           for _ in range(f)], dim=1)
        dense = torch.randn(b, 13, generator=gen)
        labels = torch.randint(0, 2, (b,), generator=gen).float()
        opt.zero_grad(set_to_none=True)
        loss = model(dense, ids, labels=labels)
        loss.backward()
        assert not model.embeddings._raw_ids_keys  # CPU keeps flat ids
        opt.step()
        model.apply_sparse_updates(lr=0.05)
        losses.append(loss.detach().clone())
    return model, losses


def test_model_two_steps_cpu_switches_on_equal_off(monkeypatch):
    on, on_losses = _train_two_steps(monkeypatch, "1")
    off, off_losses = _train_two_steps(monkeypatch, "0")
    for a, c in zip(on_losses, off_losses):
        assert torch.equal(a, c)
    assert list(on.state_dict()) == list(off.state_dict())
    for (name, p), (_, q) in zip(on.named_parameters(),
                                 off.named_parameters()):
        assert torch.equal(p, q), name
    # two different batches went through
    assert not torch.equal(on_losses[0], on_losses[1])
