"""The six dense optimizer kernels (``csrc/fused_optimizers.hip``) against
the float64 rules of ``tests/optim_refs.py``.

* SGD and multi-tensor SGD: dyadic operands, every intermediate exact in
  fp32, so ``torch.equal`` against the reference and the bf16 copy equal to
  the integer round-to-nearest-even of it.
* Adam/AdamW, Adagrad, Adadelta, FTRL: N(0, 1) operands with warm states.
  ``E(x) = max|x - ref64| / ulp32(max|ref64|)`` of the GPU result is held
  to ``4 * max(E(cpu), 1)``, ``E(cpu)`` being the project's fp32 CPU path
  of the same call, measured in the same test.
* Sizes: the quad and tail edges, exactly one full grid-stride trip
  (2048 blocks x 256 threads x 4 floats) and a second trip that 1000
  threads take, with a 3-element tail.
* Views at element offsets 1, 2, 3 of a buffer (pointers that are not
  16-byte aligned) give the bits of the same call on aligned clones and
  leave the buffer around the view alone.
"""

import pytest
import torch

import optim_refs as R
from tf_yarn_amd import ops
from tf_yarn_amd.ops import optim

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")

FULL_TRIP = 2048 * 256 * 4  # MIYARN_MAX_BLOCKS x MIYARN_BLOCK x 4 floats
SIZES = [1, 3, 4, 5, 1023, 1025, FULL_TRIP, FULL_TRIP + 4 * 1000 + 3]
assert SIZES[-2:] == [2_097_152, 2_101_155]

GDTYPES = [torch.float32, torch.bfloat16]
# (momentum buffer, nesterov, first_step); without a buffer the kernel
# reads neither flag
SGD_FLAGS = [(False, False, False), (True, False, False),
             (True, True, False), (True, False, True), (True, True, True)]
CANARY = 7.0


def _apply(rule, p, g, states, copy=None, **kw):
    """One in-place ``ops.fused_*`` call."""
    if rule == "adam":
        ops.fused_adam(p, g, *states, copy, **kw)
    elif rule == "adagrad":
        ops.fused_adagrad(p, g, *states, **kw)
    elif rule == "adadelta":
        ops.fused_adadelta(p, g, *states, **kw)
    else:
        ops.fused_ftrl(p, g, *states, **kw)


def _bound(name, got, cpu, ref64):
    """Print and assert ``E(gpu) <= 4 * max(E(cpu), 1)``."""
    e_gpu, e_cpu = R.err_ulps(got, ref64), R.err_ulps(cpu, ref64)
    print(f"E {name}: gpu {e_gpu:.3f} cpu {e_cpu:.3f}")
    assert e_gpu <= 4.0 * max(e_cpu, 1.0), \
        f"{name}: E(gpu) = {e_gpu:.3f}, E(cpu) = {e_cpu:.3f}"


def _copy_like(p):
    return torch.full(p.shape, CANARY, dtype=torch.bfloat16, device=p.device)


# ---- SGD: bit-exact ---------------------------------------------------------

def _sgd_exact_one(n, seed, mom, nesterov, first_step, gdtype):
    """Operands on the GPU and the fp32 / bf16 tensors a correct kernel
    leaves: ``(p, g, m, want_p, want_m, want_copy)``."""
    p, g, m = R.dyadic_sgd_case(n, seed)
    kw = dict(R.DYADIC_SGD_KW, nesterov=nesterov, first_step=first_step)
    p_ref, m_ref = R.sgd(p, g, m if mom else None, **kw)
    want_p = p_ref.float()
    return (p.float().cuda(), g.to(gdtype).cuda(),
            m.float().cuda() if mom else None, want_p,
            m_ref.float() if mom else None, R.rne_bf16_of(want_p), kw)


@requires_gpu
@pytest.mark.parametrize("with_copy", [False, True])
@pytest.mark.parametrize("gdtype", GDTYPES)
@pytest.mark.parametrize("mom,nesterov,first_step", SGD_FLAGS)
@pytest.mark.parametrize("n", SIZES)
def test_fused_sgd_exact(n, mom, nesterov, first_step, gdtype, with_copy):
    p, g, m, want_p, want_m, want_copy, kw = _sgd_exact_one(
        n, 0, mom, nesterov, first_step, gdtype)
    copy = _copy_like(p) if with_copy else None
    ops.fused_sgd(p, g, m, copy, **kw)
    assert torch.equal(p.cpu(), want_p)
    if mom:
        assert torch.equal(m.cpu(), want_m)
    if with_copy:
        assert torch.equal(copy.cpu().view(torch.int16),
                           want_copy.view(torch.int16))


MT_SIZES = {
    # the grid is sized by the largest tensor: short ones idle through it
    "ragged": [SIZES[-1], 3, 1024, 437, 4],
    # 30 tensors cross MT_MAX = 24: two launches
    "thirty": [(1, 3, 4, 5, 7, 64, 437, 1023, 1025, 2049)[i % 10] + i // 10
               for i in range(30)],
}


@requires_gpu
@pytest.mark.parametrize("with_copy", [False, True])
@pytest.mark.parametrize("gdtype", GDTYPES)
@pytest.mark.parametrize("mom,nesterov,first_step", SGD_FLAGS)
@pytest.mark.parametrize("sizes", sorted(MT_SIZES))
def test_fused_sgd_mt_exact(sizes, mom, nesterov, first_step, gdtype,
                            with_copy):
    cases = [_sgd_exact_one(n, i, mom, nesterov, first_step, gdtype)
             for i, n in enumerate(MT_SIZES[sizes])]
    ps = [c[0] for c in cases]
    copies = [_copy_like(p) for p in ps] if with_copy else None
    ops.fused_sgd_mt(ps, [c[1] for c in cases],
                     [c[2] for c in cases] if mom else None, copies,
                     **cases[0][6])
    for i, (p, _, m, want_p, want_m, want_copy, _) in enumerate(cases):
        assert torch.equal(p.cpu(), want_p), i
        if mom:
            assert torch.equal(m.cpu(), want_m), i
        if with_copy:
            assert torch.equal(copies[i].cpu().view(torch.int16),
                               want_copy.view(torch.int16)), i


# ---- Adam/AdamW, Adagrad, Adadelta, FTRL: random operands vs float64 -------

RULE_VARIANTS = [("adam", False, False), ("adam", False, True),
                 ("adam", True, False), ("adam", True, True),
                 ("adagrad", False, False), ("adadelta", False, False),
                 ("ftrl", False, False)]


@requires_gpu
@pytest.mark.parametrize("gdtype", GDTYPES)
@pytest.mark.parametrize("rule,adamw,with_copy", RULE_VARIANTS)
@pytest.mark.parametrize("n", SIZES)
def test_rule_vs_float64(n, rule, adamw, with_copy, gdtype):
    p, g, states, kw = R.warm_case(rule, n, adamw)
    g = g.to(gdtype)
    ref = R.RULES[rule](p.double(), g, *(s.double() for s in states), **kw)
    c_p, c_states = p.clone(), [s.clone() for s in states]
    _apply(rule, c_p, g, c_states, **kw)
    g_p, g_states = p.cuda(), [s.cuda() for s in states]
    copy = _copy_like(g_p) if with_copy else None
    _apply(rule, g_p, g.cuda(), g_states, copy, **kw)
    tag = f"{rule}{'w' if adamw else ''} n={n} " \
          f"{'bf16' if gdtype == torch.bfloat16 else 'fp32'} grads"
    _bound(f"{tag} param", g_p, c_p, ref[0])
    for name, gs, cs, r in zip(R.STATE_NAMES[rule], g_states, c_states,
                               ref[1:]):
        _bound(f"{tag} {name}", gs, cs, r)
    if with_copy:
        # taken after the update, from the value the master holds
        assert torch.equal(copy.cpu().view(torch.int16),
                           R.rne_bf16_of(g_p.cpu()).view(torch.int16))
    if rule == "ftrl":
        band = R.ftrl_band_mask(p, g, *states, **kw)
        assert torch.equal((g_p.cpu() == 0)[~band], (ref[0] == 0)[~band])


# ---- the optimizer classes ---------------------------------------------------

SHAPES = [(7, 5), (64, 64), (2, 3, 4, 4)]
STEPS = 3


def _class_inputs(dtype):
    """Start weights and per-step gradients in ``dtype``, on the CPU; the
    last parameter is channels_last (``_flat``'s ``as_strided`` branch)."""
    gen = torch.Generator().manual_seed(11)
    p0 = [torch.randn(s, generator=gen).to(dtype) for s in SHAPES]
    p0[2] = p0[2].contiguous(memory_format=torch.channels_last)
    assert not p0[2].is_contiguous()
    grads = [[torch.randn(s, generator=gen).to(dtype) for s in SHAPES]
             for _ in range(STEPS)]
    return p0, grads


def _run_class(make, p0, grads, device):
    params = [torch.nn.Parameter(p.clone().to(device)) for p in p0]
    assert not params[2].is_contiguous()
    opt = make(params)
    for gs in grads:
        for p, g in zip(params, gs):
            p.grad = g.to(device)  # contiguous: _grad_of re-lays the last
        opt.step()
    return params, opt


SGD_CLASS_KW = dict(lr=0.1, momentum=0.9, dampening=0.1, weight_decay=0.01,
                    grad_scale=0.5)


def _class_kw(rule, **extra):
    """``R.RULE_KW[rule]`` as the class's constructor takes it."""
    kw = dict(R.RULE_KW[rule], **extra)
    kw.pop("step", None)
    if rule == "adam":
        kw["betas"] = (kw.pop("beta1"), kw.pop("beta2"))
    return kw


# name -> (constructor, the class's state keys in the rule's order)
CLASS_CASES = {
    "sgd": (lambda ps: optim.FusedSGD(ps, **SGD_CLASS_KW),
            ("momentum_buffer",)),
    "adam": (lambda ps: optim.FusedAdam(ps, **_class_kw("adam")),
             ("exp_avg", "exp_avg_sq")),
    "adamw": (lambda ps: optim.FusedAdam(ps, **_class_kw("adam",
                                                         adamw=True)),
              ("exp_avg", "exp_avg_sq")),
    "adagrad": (lambda ps: optim.FusedAdagrad(ps, **_class_kw("adagrad")),
                ("sum",)),
    "adadelta": (lambda ps: optim.FusedAdadelta(ps, **_class_kw("adadelta")),
                 ("square_avg", "acc_delta")),
    "ftrl": (lambda ps: optim.FusedFtrl(
        ps, initial_accumulator_value=R.FTRL_INITIAL_ACCUM,
        **_class_kw("ftrl")), ("accum", "linear")),
}


def _class_reference(name, p0, grads):
    """``STEPS`` float64 steps of the rule behind ``CLASS_CASES[name]``:
    per parameter ``(p, *states)``."""
    out = []
    for i, p in enumerate(p0):
        p = p.double()
        if name == "sgd":
            m = torch.zeros_like(p)
            for t in range(STEPS):
                p, m = R.sgd(p, grads[t][i], m, first_step=(t == 0),
                             **SGD_CLASS_KW)
            out.append((p, m))
            continue
        rule = "adam" if name == "adamw" else name
        kw = dict(R.RULE_KW[rule])
        if rule == "adam":
            kw["adamw"] = name == "adamw"
        states = R._zero_states(rule, p)
        for t in range(STEPS):
            skw = dict(kw, step=t + 1) if rule == "adam" else kw
            p, *states = R.RULES[rule](p, grads[t][i], *states, **skw)
        out.append((p, *states))
    return out


@requires_gpu
@pytest.mark.parametrize("name", sorted(CLASS_CASES))
def test_optimizer_class_fp32_params(name):
    make, state_keys = CLASS_CASES[name]
    p0, grads = _class_inputs(torch.float32)
    ref = _class_reference(name, p0, grads)
    c_params, c_opt = _run_class(make, p0, grads, "cpu")
    g_params, g_opt = _run_class(make, p0, grads, "cuda")
    for i, (gp, cp) in enumerate(zip(g_params, c_params)):
        tag = f"Fused {name} {list(SHAPES[i])}"
        _bound(f"{tag} param", gp, cp, ref[i][0])
        for k, key in enumerate(state_keys):
            _bound(f"{tag} {key}", g_opt.state[gp][key],
                   c_opt.state[cp][key], ref[i][1 + k])


@requires_gpu
@pytest.mark.parametrize("name", ["sgd", "adam"])
def test_optimizer_class_bf16_params(name):
    """bf16 parameters: the fp32 master follows the reference and the
    parameter is the bf16 rounding of the master, bit for bit."""
    make, _ = CLASS_CASES[name]
    p0, grads = _class_inputs(torch.bfloat16)
    ref = _class_reference(name, p0, grads)
    c_params, c_opt = _run_class(make, p0, grads, "cpu")
    g_params, g_opt = _run_class(make, p0, grads, "cuda")
    for i, (gp, cp) in enumerate(zip(g_params, c_params)):
        master = g_opt.state[gp]["master"]
        _bound(f"Fused {name} bf16 {list(SHAPES[i])} master", master,
               c_opt.state[cp]["master"], ref[i][0])
        assert gp.dtype == torch.bfloat16
        assert torch.equal(gp.detach().cpu().view(torch.int16),
                           R.rne_bf16_of(master.cpu()).view(torch.int16))


# ---- alignment ---------------------------------------------------------------

ALIGN_N = 1025


def _in_buffer(t, off):
    """``t`` copied into ``buf[off : off + n]`` of a fresh GPU buffer of
    canaries; ``off`` elements past the allocation's 16-byte boundary."""
    buf = torch.full((t.numel() + 8,), CANARY, dtype=t.dtype, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[off:off + t.numel()]
    view.copy_(t)
    return buf, view


def _untouched(buf, off, n):
    return bool((buf[:off] == CANARY).all()) and \
        bool((buf[off + n:] == CANARY).all())


def _sgd_neighbours(extra, kw):
    """What ``fused_sgd`` leaves for the aligned neighbours of the
    multi-tensor call: ``(p, m, copy)`` each."""
    out = []
    for e in extra:
        p, g, m = (t.clone() for t in e)
        copy = _copy_like(p)
        ops.fused_sgd(p, g, m, copy, **kw)
        out.append((p, m, copy))
    return out


def _align_operands(kernel):
    """CPU fp32 vector-accessed tensors ``[p, *states, copy?]``, the
    gradient, and a function running the kernel on such a list."""
    n = ALIGN_N
    if kernel in ("sgd", "sgd_mt"):
        p, g, m = R.dyadic_sgd_case(n, 5)
        kw = dict(R.DYADIC_SGD_KW, nesterov=True)
        tensors = [p.float(), m.float(),
                   torch.full((n,), CANARY, dtype=torch.bfloat16)]
        if kernel == "sgd":
            def run(ts, gg):
                ops.fused_sgd(ts[0], gg, ts[1], ts[2], **kw)
        else:
            # the tensor under test between two aligned ones
            extra = [[t.float().cuda() for t in R.dyadic_sgd_case(k, 6 + k)]
                     for k in (1025, 7)]

            def run(ts, gg):
                fresh = [[t.clone() for t in e] for e in extra]
                copies = [_copy_like(e[0]) for e in fresh]
                ops.fused_sgd_mt(
                    [fresh[0][0], ts[0], fresh[1][0]],
                    [fresh[0][1], gg, fresh[1][1]],
                    [fresh[0][2], ts[1], fresh[1][2]],
                    [copies[0], ts[2], copies[1]], **kw)
                want = _sgd_neighbours(extra, kw)
                for f, c, w in zip(fresh, copies, want):
                    assert torch.equal(f[0], w[0]) and \
                        torch.equal(f[2], w[1]) and torch.equal(c, w[2])
        return tensors, g.float(), run
    p, g, states, kw = R.warm_case(kernel, n)
    tensors = [p, *states]
    if kernel == "adam":
        tensors.append(torch.full((n,), CANARY, dtype=torch.bfloat16))

        def run(ts, gg):
            ops.fused_adam(ts[0], gg, ts[1], ts[2], ts[3], **kw)
    else:
        def run(ts, gg):
            _apply(kernel, ts[0], gg, ts[1:], **kw)
    return tensors, g, run


ALIGN_CASES = [(k, which) for k, nt in (("sgd", 3), ("sgd_mt", 3),
                                        ("adam", 4), ("adagrad", 2),
                                        ("adadelta", 3), ("ftrl", 3))
               for which in range(-1, nt)]


@requires_gpu
@pytest.mark.parametrize("off", [1, 2, 3])
@pytest.mark.parametrize("kernel,which", ALIGN_CASES)
def test_misaligned_views_match_aligned_clones(kernel, which, off):
    """``which``: the index of the one misaligned tensor among
    ``[p, *states, copy]``, or -1 for all of them.  The gradient, which
    the kernels read by scalars, sits at the offset too."""
    tensors, g, run = _align_operands(kernel)
    aligned = [t.cuda() for t in tensors]
    assert all(t.data_ptr() % 16 == 0 for t in aligned)
    run(aligned, g.cuda())
    bufs, views = [], []
    for i, t in enumerate(tensors):
        buf, view = _in_buffer(t, off if which in (-1, i) else 0)
        bufs.append(buf)
        views.append(view)
    assert any(v.data_ptr() % (8 if v.dtype == torch.bfloat16 else 16)
               for v in views)
    run(views, _in_buffer(g, off)[1])
    for i, (v, a, buf) in enumerate(zip(views, aligned, bufs)):
        bits = torch.int16 if v.dtype == torch.bfloat16 else torch.int32
        assert torch.equal(v.view(bits), a.view(bits)), i
        assert _untouched(buf, off if which in (-1, i) else 0, ALIGN_N), i
