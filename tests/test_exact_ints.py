"""CPU cover for the exact-integer helper behind test_dense_exact_gpu.py."""

import pytest
import torch

import exact_ints


def test_bound_is_enforced():
    exact_ints.assert_exact(2, 2, 65536)            # 2**18: the bench depth
    exact_ints.assert_exact(2, 2, 2 ** 22 - 1)      # just below 2**24
    with pytest.raises(AssertionError, match="2\\*\\*24"):
        exact_ints.assert_exact(2, 2, 2 ** 22)      # reaches 2**24
    with pytest.raises(AssertionError, match="2\\*\\*24"):
        exact_ints.assert_exact(2, 2, 2 ** 22 - 1, extra=4)  # bias tips it
    with pytest.raises(AssertionError, match="bf16"):
        exact_ints.assert_exact(257, 1, 4)          # not a bf16 integer
    with pytest.raises(AssertionError):
        exact_ints.operands((4, 2 ** 22), (2 ** 22, 4), 2 ** 22)


def test_operands_are_small_integers_exact_in_bf16():
    a, b = exact_ints.operands((64, 33), (64, 7), 64, amax_a=2, amax_b=256)
    assert a.dtype == torch.int16 and a.abs().max() <= 2
    assert b.abs().max() <= 256 and b.abs().max() > 2
    assert set(a.unique().tolist()) == {-2, -1, 0, 1, 2}
    assert torch.equal(b.to(torch.bfloat16).double(), b.double())


def test_fp32_mm_equals_float64_at_bench_depth():
    """At K = 65536 an fp32 GEMM of the integer operands equals the
    float64 reference exactly, blocked summation order and all; so does
    the worst case the bound allows for (every product +4)."""
    k = 65536
    a, b = exact_ints.operands((k, 8), (k, 16), k, seed=1)
    ref64 = a.double().t() @ b.double()
    assert torch.equal(a.float().t() @ b.float(), ref64.float())
    assert torch.equal(ref64.float().double(), ref64)
    worst = torch.full((k, 4), 2.0)
    assert torch.equal(worst.t() @ worst, torch.full((4, 4), 4.0 * k))


def _slabs(name, B, N, M, splitk):
    """Mirror of the host-side split-K arithmetic of csrc/wgrad.hip:
    the k-steps (of 64 batch rows) each slab reduces."""
    tile, budget, cap = {"wgrad_nt128": (128, 512, 32),
                         "wgrad_nt256": (256, 256, 32)}[name]
    tiles = (N // tile) * -(-M // tile)
    if splitk <= 0:
        splitk = max(1, budget // tiles)
        if cap:
            splitk = min(cap, splitk)
    chunk = -(-(-(-B // splitk)) // 64) * 64
    return [(min(B, k + chunk) - k) // 64 for k in range(0, B, chunk)]


def test_wgrad_cases_reach_the_short_slab_and_the_clamp():
    """The GPU cases are chosen for branches of the launch arithmetic;
    show on the mirror that they reach them.  With these inputs a kernel
    that ran a short last slab to the full chunk (or dropped its last
    k-step) changes the integer sums, so exact equality turns red."""
    from test_dense_exact_gpu import _wgrad_cases
    seen = {}
    for name, B, N, M, splitk, _ in _wgrad_cases():
        slabs = _slabs(name, B, N, M, splitk)
        assert sum(slabs) * 64 == B and min(slabs) >= 1
        kinds = seen.setdefault(name, set())
        if slabs[-1] < slabs[0]:
            kinds.add("short last slab")
            if splitk == 0:
                kinds.add("short last slab, auto split")
        if splitk > B // 64:
            assert len(slabs) == B // 64
            kinds.add("clamped")
        if len(slabs) == 1:
            kinds.add("one slab")
        if B == 65536:
            kinds.add("depth")
    for name, kinds in seen.items():
        assert {"short last slab", "short last slab, auto split",
                "clamped", "one slab", "depth"} <= kinds, name
    assert _slabs("wgrad_nt128", 65 * 64, 128, 8, 0) == [3] * 21 + [2]
    assert _slabs("wgrad_nt256", 3 * 64, 256, 264, 100) == [1, 1, 1]


def test_rne_and_half_ulp():
    # bf16 spacing is 2 in [256, 512): odd integers are ties -> even code
    ref = torch.tensor([257.0, 259.0, 258.0, -257.0, 1.0, 0.0],
                       dtype=torch.float64)
    assert exact_ints.rne_bf16(ref).tolist() == [256.0, 260.0, 258.0,
                                                 -256.0, 1.0, 0.0]
    assert exact_ints.bf16_half_ulp(ref).tolist() == [
        1.0, 1.0, 1.0, 1.0, 2.0 ** -8, 0.0]
    assert exact_ints.bf16_half_ulp(
        torch.tensor([0.75], dtype=torch.float64)).item() == 2.0 ** -9
