"""CPU side of dgrad_drelu and MLPHeadFn: off the kernel's preconditions
the ops compose what ran before them, and the deep tower keeps its route."""

import pytest
import torch

import dgrad_cases
import exact_ints
from tf_yarn_amd import ops

BF16 = torch.bfloat16


@pytest.mark.parametrize("dtype", [torch.float32, BF16])
@pytest.mark.parametrize("m,k,n", [(256, 16, 16), (37, 24, 40), (5, 3, 7)])
def test_dgrad_drelu_cpu_is_the_composition(m, k, n, dtype):
    a, w, y = dgrad_cases.dgrad_operands(m, k, n, seed=m + n, saturate=False)
    _, dz_ref, db_ref = dgrad_cases.dgrad_reference(a, w, y)
    dz, db = ops.dgrad_drelu(a.to(dtype), w.to(dtype), y.to(dtype))
    assert dz.dtype == dtype and db.dtype == dtype
    # |acc| <= 4 k <= 96: no rounding in either dtype
    assert torch.equal(dz.double(), dz_ref)
    want_db = db_ref if dtype == torch.float32 \
        else exact_ints.rne_bf16(db_ref).double()
    assert torch.equal(db.double(), want_db)
    dx = a.to(dtype).matmul(w.to(dtype))
    two = ops.bias_relu_bwd(dx, y.to(dtype))
    assert torch.equal(dz, two)


def test_tower_cpu_matches_float64_autograd_and_the_modules():
    case = dgrad_cases.tower_operands()
    ref, ref_out = dgrad_cases.tower_reference(*case)
    got, out = dgrad_cases.run_tower(ops.mlp_bias_relu_head, *case, "cpu")
    assert torch.equal(out.double(), ref_out)
    for g, r in zip(got, ref):
        assert g.dtype == BF16
        assert torch.equal(g, exact_ints.rne_bf16(r))

    def modules(x, weights, biases, w_head, b_head):
        h = x
        for w, b in zip(weights[:-1], biases[:-1]):
            h = ops.linear_bias_relu(h, w, b)
        return ops.linear_bias_relu_head(h, weights[-1], biases[-1], w_head,
                                         b_head)

    old, old_out = dgrad_cases.run_tower(modules, *case, "cpu")
    assert torch.equal(out, old_out)
    for g, o in zip(got, old):
        assert torch.equal(g, o)


def test_routing_needs_the_switch_the_batch_and_a_routed_shape(monkeypatch):
    weights = [torch.empty(64, 48), torch.empty(32, 64), torch.empty(16, 32)]
    monkeypatch.setattr(ops, "_fused_dgrad_shape_routed",
                        lambda k, n: (k, n) == (32, 64))
    monkeypatch.delenv("MIYARN_FUSED_DGRAD", raising=False)
    assert ops.fused_dgrad_enabled()
    assert ops.mlp_head_routed(torch.empty(256, 48), weights)
    assert not ops.mlp_head_routed(torch.empty(64, 48), weights)
    assert not ops.mlp_head_routed(torch.empty(0, 48), weights)
    # layer 0's dgrad is never fused: its input is no ReLU output
    monkeypatch.setattr(ops, "_fused_dgrad_shape_routed",
                        lambda k, n: (k, n) == (64, 48))
    assert not ops.mlp_head_routed(torch.empty(256, 48), weights)
    monkeypatch.setattr(ops, "_fused_dgrad_shape_routed", lambda k, n: True)
    for off in ("0", ""):
        monkeypatch.setenv("MIYARN_FUSED_DGRAD", off)
        assert not ops.fused_dgrad_enabled()
        assert not ops.mlp_head_routed(torch.empty(256, 48), weights)
    monkeypatch.setenv("MIYARN_FUSED_DGRAD", "1")
    assert ops.mlp_head_routed(torch.empty(256, 48), weights)


def test_deep_tower_cpu_takes_the_modules(monkeypatch):
    from tf_yarn_amd.models.wide_deep import WideAndDeep
    monkeypatch.setattr(ops, "_fused_dgrad_shape_routed", lambda k, n: True)
    monkeypatch.setenv("MIYARN_FUSED_DGRAD", "1")
    calls = []
    monkeypatch.setattr(ops, "mlp_bias_relu_head",
                        lambda *a: calls.append(1))
    torch.manual_seed(0)
    model = WideAndDeep(table_sizes=[50] * 26, embedding_dim=16,
                        hidden=(64, 32))
    deep_in = torch.randn(256, 432)
    out = model._deep_tower(deep_in)
    assert not calls
    assert torch.equal(out, model.head(model.mlp(deep_in)))
