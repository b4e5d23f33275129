"""CPU checks of ``tests/optim_refs.py``: the float64 rules against
``torch.optim`` in float64, the integer bf16 rounding against torch's CPU
cast, and the exactness the dyadic SGD operands promise.  These validate
the references, not the kernels."""

import numpy as np
import pytest
import torch

from tf_yarn_amd import ops

import optim_refs as R

N = 257


def _grads(steps, seed):
    gen = torch.Generator().manual_seed(seed)
    p0 = torch.randn(N, generator=gen, dtype=torch.float64)
    gs = [torch.randn(N, generator=gen, dtype=torch.float64)
          for _ in range(steps)]
    return p0, gs


def _run_torch(opt_cls, p0, gs, grad_scale, **kw):
    p = p0.clone().requires_grad_(True)
    opt = opt_cls([p], **kw)
    for g in gs:
        p.grad = g * grad_scale
        opt.step()
    return p.detach(), opt.state[p]


def _close(a, b):
    torch.testing.assert_close(a, b, rtol=1e-12, atol=0.0)


@pytest.mark.parametrize("momentum,dampening,nesterov", [
    (0.0, 0.0, False), (0.9, 0.0, False), (0.9, 0.25, False),
    (0.9, 0.0, True)])
def test_sgd_rule_vs_torch_float64(momentum, dampening, nesterov):
    p0, gs = _grads(3, 0)
    want, state = _run_torch(torch.optim.SGD, p0, gs, 0.5, lr=0.1,
                             momentum=momentum, dampening=dampening,
                             weight_decay=0.01, nesterov=nesterov)
    p, m = p0, (torch.zeros_like(p0) if momentum else None)
    for i, g in enumerate(gs):
        p, m = R.sgd(p, g, m, lr=0.1, momentum=momentum,
                     dampening=dampening, weight_decay=0.01,
                     nesterov=nesterov, first_step=(i == 0), grad_scale=0.5)
    _close(p, want)
    if momentum:
        _close(m, state["momentum_buffer"])


def test_sgd_mt_rule_is_the_rule_per_tensor():
    kw = dict(lr=0.1, momentum=0.9, dampening=0.1, weight_decay=0.01,
              grad_scale=0.5)
    cases = [_grads(2, s) for s in (1, 2, 3)]
    ps = [c[0] for c in cases]
    gs = [c[1][0] for c in cases]
    ms = [c[1][1] for c in cases]
    got_p, got_m = R.sgd_mt(ps, gs, ms, **kw)
    for i in range(3):
        p, m = R.sgd(ps[i], gs[i], ms[i], **kw)
        assert torch.equal(got_p[i], p) and torch.equal(got_m[i], m)
    got_p, got_m = R.sgd_mt(ps, gs, None, **kw)
    assert got_m is None
    assert torch.equal(got_p[0], R.sgd(ps[0], gs[0], None, **kw)[0])


@pytest.mark.parametrize("adamw", [False, True])
def test_adam_rule_vs_torch_float64(adamw):
    p0, gs = _grads(3, 4)
    cls = torch.optim.AdamW if adamw else torch.optim.Adam
    want, state = _run_torch(cls, p0, gs, 0.5, lr=0.01, betas=(0.9, 0.99),
                             eps=1e-8, weight_decay=0.01)
    p, m, v = p0, torch.zeros_like(p0), torch.zeros_like(p0)
    for i, g in enumerate(gs):
        p, m, v = R.adam(p, g, m, v, lr=0.01, beta1=0.9, beta2=0.99,
                         eps=1e-8, weight_decay=0.01, adamw=adamw,
                         step=i + 1, grad_scale=0.5)
    _close(p, want)
    _close(m, state["exp_avg"])
    _close(v, state["exp_avg_sq"])


def test_adagrad_rule_vs_torch_float64():
    p0, gs = _grads(3, 5)
    want, state = _run_torch(torch.optim.Adagrad, p0, gs, 0.5, lr=0.05,
                             eps=1e-10, weight_decay=0.01)
    p, acc = p0, torch.zeros_like(p0)
    for g in gs:
        p, acc = R.adagrad(p, g, acc, lr=0.05, eps=1e-10,
                           weight_decay=0.01, grad_scale=0.5)
    _close(p, want)
    _close(acc, state["sum"])


def test_adadelta_rule_vs_torch_float64():
    p0, gs = _grads(3, 6)
    want, state = _run_torch(torch.optim.Adadelta, p0, gs, 0.5, lr=1.0,
                             rho=0.9, eps=1e-6, weight_decay=0.01)
    p, sq, ad = p0, torch.zeros_like(p0), torch.zeros_like(p0)
    for g in gs:
        p, sq, ad = R.adadelta(p, g, sq, ad, lr=1.0, rho=0.9, eps=1e-6,
                               weight_decay=0.01, grad_scale=0.5)
    _close(p, want)
    _close(sq, state["square_avg"])
    _close(ad, state["acc_delta"])


def test_ftrl_rule_vs_ops_rule_float64():
    p0, gs = _grads(3, 7)
    w, n, z = p0, torch.full_like(p0, 0.1), torch.zeros_like(p0)
    w2, n2, z2 = w, n, z
    for g in gs:
        w, n, z = R.ftrl(w, g, n, z, lr=0.05, l1=0.3, l2=0.001,
                         grad_scale=0.5)
        n2, z2, w2 = ops._ftrl_rule(g * 0.5, n2, z2, w2, 0.05, 0.3, 0.001)
        _close(w, w2)
        _close(n, n2)
        _close(z, z2)
        assert torch.equal(w == 0, w2 == 0)
    assert 0 < int((w == 0).sum()) < N  # both branches of the rule ran


# ---- bf16 rounding ---------------------------------------------------------

def test_pattern_sets():
    bits = R.f32_patterns()
    assert bits.dtype == np.uint32 and bits.shape == (393216,)
    assert len(np.unique(bits)) == 393216
    nan = R.is_nan_bits(bits)
    assert int(nan.sum()) == 1534
    t = R.f32_from_bits(bits)
    assert np.array_equal(R.bits_of(t), bits)
    assert np.array_equal(torch.isnan(t).numpy(), nan)
    for special in (0x7f800001, 0x7fffffff, 0xffffffff, 0x7f7fffff,
                    0x00000001, 0x007fffff, 0x80000000, 0x7f800000):
        assert special in bits
    b = R.bf16_patterns()
    assert b.dtype == np.uint16 and len(np.unique(b)) == 65536
    assert np.array_equal(R.bits_of(R.bf16_from_bits(b)), b)


def test_integer_rne_vs_torch_cpu_cast_on_every_non_nan_pattern():
    bits = R.f32_patterns()
    finite = bits[~R.is_nan_bits(bits)]
    assert finite.shape == (391682,)
    want = R.bits_of(R.f32_from_bits(finite).to(torch.bfloat16))
    assert np.array_equal(R.rne_bf16_bits(finite), want)


def test_integer_rne_known_values():
    def one(x):
        return int(R.rne_bf16_bits(np.array([x], dtype=np.uint32))[0])
    assert one(0x3f800000) == 0x3f80
    assert one(0x3f808000) == 0x3f80   # tie, kept bit even: down
    assert one(0x3f818000) == 0x3f82   # tie, kept bit odd: up
    assert one(0x3f808001) == 0x3f81
    assert one(0x3f807fff) == 0x3f80
    assert one(0x7f7fffff) == 0x7f80   # overflow to +Inf
    assert one(0xff7fffff) == 0xff80
    assert one(0x00008000) == 0x0000   # denormal tie to even (zero)
    assert one(0x00008001) == 0x0001
    assert one(0x007fffff) == 0x0080   # largest denormal -> smallest normal
    with pytest.raises(AssertionError):
        one(0x7fffffff)


def test_unguarded_rounding_breaks_twelve_nans():
    """The arithmetic the guard in ``f32_to_bf16`` protects: without it 12
    of the set's 1,534 NaNs become +-Inf or +-0."""
    bits = R.f32_patterns()
    nan = bits[R.is_nan_bits(bits)].astype(np.uint64)
    out = ((nan + 0x7fff + ((nan >> 16) & 1)) >> 16) & 0xffff
    still_nan = (out & 0x7fff) > 0x7f80
    assert int((~still_nan).sum()) == 12
    assert set(out[~still_nan].tolist()) == {0x7f80, 0xff80, 0x8000, 0x0000}


def test_rne_bf16_of_tensor():
    t = R.f32_from_bits(np.array([0x3f808001, 0x7fffffff, 0x7f800001,
                                  0xffffffff, 0x7f7fffff], dtype=np.uint32))
    assert R.bits_of(R.rne_bf16_of(t)).tolist() == \
        [0x3f81, 0x7fc0, 0x7fc0, 0x7fc0, 0x7f80]


# ---- dyadic operands --------------------------------------------------------

def test_dyadic_values():
    x = R.dyadic(5000, 3)
    k = x * 8
    assert torch.equal(k, k.round()) and k.abs().max() <= 64
    assert len(torch.unique(k)) == 129
    assert torch.equal(x.to(torch.bfloat16).double(), x)  # exact in bf16
    assert not torch.equal(x[:2500], x[2500:])
    assert torch.equal(R.dyadic(5000, 3), x)


@pytest.mark.parametrize("mom", [False, True])
@pytest.mark.parametrize("nesterov", [False, True])
@pytest.mark.parametrize("first_step", [False, True])
def test_dyadic_sgd_is_exact_in_fp32(mom, nesterov, first_step):
    """The float64 result round-trips through fp32, and the project's fp32
    CPU path, a different chain of roundings than any kernel, lands on it
    bit for bit; the bf16 copy is a real rounding."""
    p, g, m = R.dyadic_sgd_case(4099)
    kw = dict(R.DYADIC_SGD_KW, nesterov=nesterov, first_step=first_step)
    p_ref, m_ref = R.sgd(p, g, m if mom else None, **kw)
    R.assert_f32_exact(p_ref)
    p32, m32 = p.float(), m.float()
    copy = torch.empty(p.numel(), dtype=torch.bfloat16)
    for gin in (g.float(), g.to(torch.bfloat16)):
        pp, mm = p32.clone(), m32.clone()
        ops.fused_sgd(pp, gin, mm if mom else None, copy, **kw)
        assert torch.equal(pp, p_ref.float())
        if mom:
            R.assert_f32_exact(m_ref)
            assert torch.equal(mm, m_ref.float())
        assert torch.equal(copy, R.rne_bf16_of(p_ref.float()))
    assert not torch.equal(copy.double(), p_ref)  # rounding happens


# ---- warm cases, the error measure, the FTRL band ----------------------------

@pytest.mark.parametrize("rule", sorted(R.RULES))
def test_warm_case_states_are_warm(rule):
    p, g, states, kw = R.warm_case(rule, 1025)
    assert p.dtype == g.dtype == torch.float32
    assert len(states) == len(R.STATE_NAMES[rule])
    for s in states:
        assert s.dtype == torch.float32 and int((s != 0).sum()) > 1000
    assert R.warm_case(rule, 1025)[0] is p  # cached


def test_err_ulps():
    ref = torch.tensor([1.0, -3.0, 0.25], dtype=torch.float64)
    assert R.err_ulps(ref.float(), ref) == 0.0
    x = ref.clone()
    x[2] += 3 * 2.0 ** -22  # ulp32(3.0) = 2**-22
    assert R.err_ulps(x, ref) == 3.0
    assert R.ulp32(1.0) == 2.0 ** -23 and R.ulp32(-0.75) == 2.0 ** -24


@pytest.mark.parametrize("n", [1025, 2_097_152, 2_101_155])
def test_ftrl_band_leaves_out_at_most_a_thousandth(n):
    """The condition on ``WARM_SEED``: outside the band the fp32 paths must
    reproduce the reference's set of zero weights, so the band may hide at
    most 0.1 % of the elements.  The fp32 CPU path agrees outside it."""
    p, g, (acc, lin), kw = R.warm_case("ftrl", n)
    band = R.ftrl_band_mask(p, g, acc, lin, **kw)
    assert int(band.sum()) <= n // 1000
    w_ref = R.ftrl(p.double(), g, acc.double(), lin.double(), **kw)[0]
    zeros = int((w_ref == 0).sum())
    assert 0 < zeros < n
    pp, aa, ll = p.clone(), acc.clone(), lin.clone()
    ops.fused_ftrl(pp, g, aa, ll, **kw)
    assert torch.equal((pp == 0)[~band], (w_ref == 0)[~band])
