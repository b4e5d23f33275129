"""dgrad_drelu (csrc/dgrad_drelu.hip) and MLPHeadFn on the GPU.

Integer operands (exact_ints.py) make the float64 reference the only
correct answer, so those comparisons are ``torch.equal``; the N(0, 1) case
carries the fp32 dot-product bound written beside it.
"""

import pytest
import torch

import dgrad_cases
import exact_ints
from tf_yarn_amd import ops

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")

BF16 = torch.bfloat16

# (M, K, N), each the smallest that reaches one branch
EXACT_SHAPES = [
    (256, 16, 16),      # the minima
    (256, 64, 256),     # no masking anywhere
    (768, 48, 16),      # tail-only k-step
    (768, 80, 432),     # tail in the second step, two ragged column tiles
    (2048, 432, 272),   # XCD-grouped map, last column tile 16 wide
    (2304, 80, 272),    # 18 row tiles, plain map
    (512, 256, 512),    # the model's two shapes
    (512, 512, 1024),
]

_cache = {}


def _case(m, k, n):
    """Device operands and the float64 reference, computed once per shape
    and never modified."""
    key = (m, k, n)
    if key not in _cache:
        a, w, y = dgrad_cases.dgrad_operands(m, k, n, seed=m + k + n)
        acc, dz_ref, db_ref = dgrad_cases.dgrad_reference(a, w, y)
        dev = [t.to(BF16).cuda() for t in (a, w, y)]
        _cache[key] = (dev, acc, dz_ref, db_ref)
    return _cache[key]


@requires_gpu
@pytest.mark.parametrize("m,k,n", EXACT_SHAPES)
def test_exact(m, k, n):
    (a, w, y), acc, dz_ref, db_ref = _case(m, k, n)
    if k >= 256:
        # the saturated corner needs more than 8 bits: the bf16 rounding
        # of dz and of dbias is exercised, ties (odd multiples of half an
        # ulp) included
        corner = acc[:8, :24]
        assert corner.abs().max() > 512
        assert (exact_ints.rne_bf16(acc).double() != acc).any()
        lost = acc - exact_ints.rne_bf16(acc).double()
        assert (lost.abs() == exact_ints.bf16_half_ulp(acc))[acc != 0].any()
        assert (exact_ints.rne_bf16(db_ref).double() != db_ref).any()
    for dbias_bf16 in (False, True):
        dz, db = ops._C.dgrad_drelu(a, w, y, dbias_bf16)
        assert dz.shape == (m, n) and dz.dtype == BF16
        assert db.shape == (n,)
        assert torch.equal(dz.cpu().double(), dz_ref)
        if dbias_bf16:
            assert db.dtype == BF16
            assert torch.equal(db.cpu(), exact_ints.rne_bf16(db_ref))
        else:
            assert db.dtype == torch.float32
            assert torch.equal(db.cpu().double(), db_ref)
        # the path it replaces: integers make the library exact too
        dz2, db2 = ops._C.bias_relu_bwd_db(a.matmul(w), y, dbias_bf16)
        assert torch.equal(dz, dz2) and torch.equal(db, db2)
        # two calls agree to the bit
        dz3, db3 = ops._C.dgrad_drelu(a, w, y, dbias_bf16)
        assert torch.equal(dz, dz3) and torch.equal(db, db3)


@requires_gpu
@pytest.mark.parametrize("fill", [0.0, 3.0], ids=["all_zero", "all_positive"])
def test_uniform_y(fill):
    m, k, n = 768, 80, 432
    (a, w, _), acc, _, _ = _case(m, k, n)
    y = torch.full((m, n), fill, dtype=BF16, device="cuda")
    dz, db = ops._C.dgrad_drelu(a, w, y, False)
    want = exact_ints.rne_bf16(acc).double() if fill > 0 \
        else torch.zeros_like(acc)
    assert torch.equal(dz.cpu().double(), want)
    assert torch.equal(db.cpu().double(), want.sum(0))


@requires_gpu
@pytest.mark.parametrize("m", [4096, 2304])
def test_position_coded(m):
    """Row block i of dz_next is the constant i + 1 and column n of w picks
    one k with weight n % 5 + 1, so acc[r, n] = (r // 256 + 1) * (n % 5 + 1)
    names its row tile and, with the mask below, its place: y passes where
    (3 r + 5 n + r // 256 + 7 (n // 256)) % 11 < 6, a pattern no other row,
    column, row tile or column tile shares.  4096 = 32 row tiles takes the
    grouped map past its first group of 8; 2304 = 18 takes the plain map."""
    k, n = 64, 528
    rows = torch.arange(m) // 256 + 1
    a = rows.unsqueeze(1).expand(m, k).float().contiguous()
    cols = torch.arange(n)
    w = torch.zeros(k, n)
    w[cols % k, cols] = (cols % 5 + 1).float()
    r = torch.arange(m).unsqueeze(1)
    c = cols.unsqueeze(0)
    y = ((3 * r + 5 * c + r // 256 + 7 * (c // 256)) % 11 < 6).float()
    acc = rows.unsqueeze(1).double() * (cols % 5 + 1).unsqueeze(0).double()
    assert acc.max() <= exact_ints.BF16_INT_MAX
    exact_ints.assert_exact(int(acc.max()), 1, m)
    ref = acc * y.double()
    dz, db = ops._C.dgrad_drelu(a.to(BF16).cuda(), w.to(BF16).cuda(),
                                y.to(BF16).cuda(), False)
    assert torch.equal(dz.cpu().double(), ref)
    assert torch.equal(db.cpu().double(), ref.sum(0))


@requires_gpu
def test_bounded_normal_operands():
    """N(0, 1) operands at the model's larger shape.  Where y > 0,
    |dz - ref| <= delta + half a bf16 ulp at (|ref| + delta) with
    delta = (K + 1) 2^-24 (|dz_next| @ |w|), the fp32 dot-product bound in
    any order; elsewhere dz is exactly zero.  The fp32 dbias is within
    M 2^-24 sum|dz| of the float64 column sums of the kernel's own dz."""
    m, k, n = 512, 512, 1024
    gen = torch.Generator().manual_seed(1024)
    a = torch.randn(m, k, generator=gen).to(BF16)
    w = torch.randn(k, n, generator=gen).to(BF16)
    y = dgrad_cases.mixed_y(m, n, gen).to(BF16)
    ref = a.double() @ w.double()
    delta = (k + 1) * 2.0 ** -24 * (a.double().abs() @ w.double().abs())
    dz, db = ops._C.dgrad_drelu(a.cuda(), w.cuda(), y.cuda(), False)
    dz = dz.cpu().double()
    keep = y.double() > 0
    err = (dz - ref).abs()
    bound = delta + exact_ints.bf16_half_ulp(ref.abs() + delta)
    print("max err / bound where kept:", (err / bound)[keep].max().item())
    assert (err <= bound)[keep].all()
    assert (dz[~keep] == 0).all()
    sums = dz.sum(0)
    db_bound = m * 2.0 ** -24 * dz.abs().sum(0)
    db_err = (db.cpu().double() - sums).abs()
    print("max dbias err / bound:", (db_err / db_bound).max().item())
    assert (db_err <= db_bound).all()


# ---- the tower ---------------------------------------------------------------

@requires_gpu
def test_tower_matches_float64_autograd_and_switch_off(monkeypatch):
    """ops.mlp_bias_relu_head at 256 x 48 -> 64 -> 32 -> 16 -> 1 with every
    hidden dgrad sent to the fused kernel: each gradient is the float64
    autograd gradient rounded once, and the MIYARN_FUSED_DGRAD=0 run's bit
    for bit."""
    case = dgrad_cases.tower_operands()
    ref, ref_out = dgrad_cases.tower_reference(*case)
    monkeypatch.setattr(ops, "_fused_dgrad_shape_routed", lambda k, n: True)
    fused_calls = []
    real = ops.dgrad_drelu
    monkeypatch.setattr(
        ops, "dgrad_drelu",
        lambda dz, w, y: fused_calls.append(tuple(w.shape)) or real(dz, w, y))
    monkeypatch.setenv("MIYARN_FUSED_DGRAD", "1")
    on, out = dgrad_cases.run_tower(ops.mlp_bias_relu_head, *case, "cuda")
    assert fused_calls == [(16, 32), (32, 64)]
    monkeypatch.setenv("MIYARN_FUSED_DGRAD", "0")
    off, out_off = dgrad_cases.run_tower(ops.mlp_bias_relu_head, *case,
                                         "cuda")
    assert len(fused_calls) == 2
    assert torch.equal(out.cpu().double(), ref_out)
    assert torch.equal(out, out_off)
    for g, o, r in zip(on, off, ref):
        assert g.dtype == BF16
        assert torch.equal(g.cpu(), exact_ints.rne_bf16(r))
        assert torch.equal(g, o)


def _model_grads(monkeypatch, batch, route):
    from tf_yarn_amd.models.synthetic import synthetic_criteo_batch
    from tf_yarn_amd.models.wide_deep import WideAndDeep
    monkeypatch.setattr(ops, "_fused_dgrad_shape_routed",
                        lambda k, n: route)
    calls = {"tower": 0, "head": 0}
    real_tower, real_head = ops.mlp_bias_relu_head, ops.linear_bias_relu_head
    monkeypatch.setattr(
        ops, "mlp_bias_relu_head",
        lambda *a: calls.__setitem__("tower", calls["tower"] + 1)
        or real_tower(*a))
    monkeypatch.setattr(
        ops, "linear_bias_relu_head",
        lambda *a: calls.__setitem__("head", calls["head"] + 1)
        or real_head(*a))
    torch.manual_seed(7)
    sizes = [100] * 26
    model = WideAndDeep(table_sizes=sizes, embedding_dim=16,
                        hidden=(64, 32, 16), compute_dtype=BF16).cuda()
    dense, ids, labels = synthetic_criteo_batch(batch, sizes, device="cuda",
                                                seed=1)
    loss = model(dense, ids, labels=labels)
    loss.backward()
    grads = {name: p.grad.clone() for name, p in model.named_parameters()
             if p.grad is not None}
    return calls, loss.detach(), grads, list(model.state_dict())


@requires_gpu
def test_deep_tower_routes(monkeypatch):
    """At batch 256 with a routed shape the model's tower is one node; at
    batch 64, with the switch off, or with no routed shape it takes the
    route it took before, and gives that route's results."""
    monkeypatch.setenv("MIYARN_FUSED_DGRAD", "1")
    calls, loss, grads, keys = _model_grads(monkeypatch, 256, True)
    assert calls == {"tower": 1, "head": 0}
    monkeypatch.setenv("MIYARN_FUSED_DGRAD", "0")
    calls0, loss0, grads0, keys0 = _model_grads(monkeypatch, 256, True)
    assert calls0 == {"tower": 0, "head": 1}
    assert keys == keys0 and grads.keys() == grads0.keys()
    # the forward runs the same kernels either way
    assert torch.equal(loss, loss0)
    monkeypatch.setenv("MIYARN_FUSED_DGRAD", "1")
    calls, _, _, _ = _model_grads(monkeypatch, 256, False)
    assert calls == {"tower": 0, "head": 1}
    calls, loss64, grads64, _ = _model_grads(monkeypatch, 64, True)
    assert calls == {"tower": 0, "head": 1}
    monkeypatch.setenv("MIYARN_FUSED_DGRAD", "0")
    calls, loss64_0, grads64_0, _ = _model_grads(monkeypatch, 64, True)
    assert calls == {"tower": 0, "head": 1}
    assert torch.equal(loss64, loss64_0)
    for name in grads64:
        assert torch.equal(grads64[name], grads64_0[name]), name
