"""Exact-arithmetic tests of the dense MLP kernels at ragged shapes.

Operands are small integers (see exact_ints.py), so a correct kernel
equals the float64 CPU reference bit for bit and every GEMM, reduction
and epilogue comparison below is ``torch.equal``.  Only the library-backed
dx/dw (section 3) and the transcendental BCE head (section 6) carry a
bound, derived next to each assertion.

Each shape is the smallest that reaches one branch of a kernel or of its
host-side launch arithmetic; the comment beside it names the branch.
"""

import pytest
import torch

import exact_ints
from tf_yarn_amd import ops

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")

F32, BF16 = torch.float32, torch.bfloat16


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _dev(t, dtype):
    return t.to(dtype).cuda()


# ---- 1. split-K MFMA weight gradients --------------------------------------

BK = 64  # k-step of both kernels (B % 64 == 0 is their precondition)


def _wgrad_cases():
    cases = []
    for name, n0, ms in (("wgrad_nt128", 128, (8, 136, 432)),
                         ("wgrad_nt256", 256, (8, 264, 432))):
        # B = 65 k-steps: auto split-K leaves a short last slab (22 slabs
        # of 3 steps, the last of 2); so does splitk=4 (17+17+17+14 steps)
        cases += [(name, 65 * BK, n0, ms[0], sk, False) for sk in (0, 4)]
        # B = 3 k-steps: splitk=2 -> slabs of 2+1 steps (short last slab),
        # splitk=100 > B/BK must be clamped to 3 by the host
        cases += [(name, 3 * BK, n0, ms[1], sk, False)
                  for sk in (1, 2, 3, 100)]
        cases.append((name, BK, n0, ms[0], 0, False))  # one k-step in all
        # M edges (masked column tail: 8 = one
        # quad pair, tile+8, 432 = the model's first layer), 3+2 steps
        cases += [(name, 5 * BK, n0, m, 2, False) for m in ms]
        cases.append((name, 5 * BK, 2 * n0, ms[-1], 0, False))  # 2 N-tiles
        cases.append((name, 5 * BK, n0, ms[-1], 3, True))       # bf16 out
        cases.append((name, 65536, n0, ms[0], 0, False))  # workload depth
    return cases


@requires_gpu
@pytest.mark.parametrize("name,B,N,M,splitk,out_bf16", _wgrad_cases())
def test_wgrad_exact(name, B, N, M, splitk, out_bf16):
    # the bf16-output case draws from +-16 so that sums pass 256 and the
    # output rounding (ties included) is really exercised
    amax = 16 if out_bf16 else 2
    dy, x = exact_ints.operands((B, N), (B, M), B, amax_a=amax,
                                amax_b=amax, seed=B + N + M + splitk)
    out = getattr(ops._C, name)(_dev(dy, BF16), _dev(x, BF16), splitk,
                                out_bf16)
    ref = dy.double().t() @ x.double()
    assert out.shape == (N, M)
    if out_bf16:
        assert out.dtype == BF16
        assert (ref.abs() > 2 * exact_ints.BF16_INT_MAX).any()
        assert torch.equal(out.cpu(), exact_ints.rne_bf16(ref))
    else:
        assert out.dtype == F32
        assert torch.equal(out.cpu(), ref.float())


@requires_gpu
@pytest.mark.parametrize("name,N,M", [("wgrad_nt128", 256, 432),
                                      ("wgrad_nt256", 512, 432)])
def test_wgrad_position_coded(name, N, M):
    """dy[b, n] = 1 only at b = b0(n), so dW[n, m] = x[b0(n), m]: every
    output entry names the single (k, m) it must have come from.  Two
    codes of x between them identify (b mod 64, b div 64, m mod 16);
    a swap of equal-looking tiles, fragments or k-slabs changes one."""
    B = 5 * BK
    n_idx = torch.arange(N)
    b0 = (n_idx * 37 + 11) % B          # 37 coprime to 320: all slabs hit
    dy = torch.zeros(B, N)
    dy[b0, n_idx] = 1.0
    b = torch.arange(B).unsqueeze(1)
    m = torch.arange(M).unsqueeze(0)
    codes = ((b % 64) * 4 + m % 4 - 128,
             (m % 16) * 16 + (b // 64) * 3 + (m // 16) % 3 - 128)
    for x in codes:
        assert x.abs().max() <= exact_ints.BF16_INT_MAX
        x = x.float()
        for splitk, out_bf16 in ((2, False), (0, True)):
            # called the way LinearBiasReLU.backward does
            out = getattr(ops._C, name)(_dev(dy, BF16), _dev(x, BF16),
                                        splitk, out_bf16)
            assert torch.equal(out.float().cpu(), x[b0])


# ---- 2. gemm_bt -------------------------------------------------------------

@requires_gpu
@pytest.mark.parametrize("epilogue", [False, True])
@pytest.mark.parametrize("M,K,N", [
    (256, 16, 16),      # plain map, 1 row tile; K = N = 16: the minimum
    (256, 432, 432),    # plain map; 6 full k-steps + a 48 tail; ragged N
    (768, 48, 16),      # plain map, 3 row tiles; K < 64: tail-only step
    (768, 64, 256),     # K and N exactly one tile: no masking anywhere
    (768, 80, 432),     # tail of 16 in the SECOND k-step; 2 ragged N tiles
    (2048, 64, 16),     # XCD-grouped map (8 row tiles), one column tile
    (2048, 48, 432),    # XCD-grouped, 2 column tiles, K < 64
    (2048, 80, 256),    # XCD-grouped, K tail
    (2048, 432, 272),   # XCD-grouped, second column tile only 16 wide
    (2304, 16, 256),    # plain map, 9 row tiles (9 % 8 != 0)
    (2304, 432, 432),   # plain map, 9 x 2 tiles, ragged everywhere
    (2304, 80, 272),
])
def test_gemm_bt_exact(M, K, N, epilogue):
    a, b = exact_ints.operands((M, K), (N, K), K, extra=8,
                               seed=M + K + N)
    bias = exact_ints.ints((N,), 8, _gen(N))
    ref = a.double() @ b.double().t()
    if epilogue:
        ref = torch.relu(ref + bias.double())
    out = ops._C.gemm_bt(_dev(a, BF16), _dev(b, BF16),
                         _dev(bias, BF16) if epilogue else None, epilogue)
    assert out.shape == (M, N) and out.dtype == BF16
    assert torch.equal(out.cpu(), exact_ints.rne_bf16(ref))


@requires_gpu
@pytest.mark.parametrize("M,N", [(4096, 272), (2048, 528), (2304, 272)])
def test_gemm_bt_position_coded(M, N):
    """Row block i of A is the constant i + 1 and B[n] picks one k with
    weight n % 5 + 1, so C[r, n] = (r // 256 + 1) * (n % 5 + 1): a block
    map that sends a tile to the wrong row block or column tile shows.
    4096 = 16 row tiles takes the grouped map past its first group of 8;
    2304 takes the plain map."""
    K = 64
    rows = torch.arange(M) // 256 + 1
    a = rows.unsqueeze(1).expand(M, K).float().contiguous()
    n = torch.arange(N)
    b = torch.zeros(N, K)
    b[n, n % K] = (n % 5 + 1).float()
    ref = rows.unsqueeze(1).double() * (n % 5 + 1).unsqueeze(0).double()
    assert ref.max() <= exact_ints.BF16_INT_MAX
    out = ops._C.gemm_bt(_dev(a, BF16), _dev(b, BF16), None, False)
    assert torch.equal(out.cpu(), exact_ints.rne_bf16(ref))


# ---- 3. lt_linear and the LinearBiasReLU routing ---------------------------

@requires_gpu
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("M,K,N", [(4096, 432, 1024), (300, 432, 1024),
                                   (64, 512, 256), (7, 64, 128),
                                   (1, 16, 16)])
def test_lt_linear_exact(M, K, N, with_bias, relu):
    x, w = exact_ints.operands((M, K), (N, K), K, extra=8, seed=M + N)
    bias = exact_ints.ints((N,), 8, _gen(K))
    ref = x.double() @ w.double().t()
    if with_bias:
        ref = ref + bias.double()
    if relu:
        ref = torch.relu(ref)
    y = ops._C.lt_linear(_dev(x, BF16), _dev(w, BF16),
                         _dev(bias, BF16) if with_bias else None, relu)
    assert y.shape == (M, N) and y.dtype == BF16
    # fp32 compute on integers is exact; the bf16 store rounds once
    assert torch.equal(y.cpu(), exact_ints.rne_bf16(ref))


@requires_gpu
@pytest.mark.parametrize("N", [24, 10])   # 10: no fused dx+dbias kernel
@pytest.mark.parametrize("K", [13, 20])
@pytest.mark.parametrize("B", [1, 63, 100])
def test_linear_bias_relu_default_routing_ragged(B, K, N):
    """Shapes outside every custom kernel's preconditions, through the
    default routing, forward and backward, against float64 autograd."""
    gen = _gen(B * 1000 + K * 10 + N)
    exact_ints.assert_exact(3, 3, K, extra=3)
    x = exact_ints.ints((B, K), 3, gen)
    w = exact_ints.ints((N, K), 3, gen)
    bias = exact_ints.ints((N,), 3, gen)
    g = exact_ints.ints((B, N), 2, gen)
    exact_ints.assert_exact(2, 3, max(B, N))

    xr, wr, br = (t.double().requires_grad_(True) for t in (x, w, bias))
    yr = torch.relu(xr @ wr.t() + br)
    yr.backward(g.double())

    xg, wg, bg = (_dev(t, BF16).requires_grad_(True) for t in (x, w, bias))
    y = ops.linear_bias_relu(xg, wg, bg)
    y.backward(_dev(g, BF16))

    # |x.w + b| <= 3*3*20 + 3 < 256: y, and so the ReLU mask, dz and the
    # column sums of dz are exact in bf16 on every path
    assert torch.equal(y.detach().cpu(), exact_ints.rne_bf16(yr.detach()))
    assert torch.equal(bg.grad.cpu(), exact_ints.rne_bf16(br.grad))
    # dx and dw come from library GEMMs on bf16 operands: exact products,
    # one rounding of the result to bf16, so at most half a bf16 ulp of
    # the reference value (and exact while |ref| <= 256)
    for got, ref in ((xg.grad, xr.grad), (wg.grad, wr.grad)):
        err = (got.double().cpu() - ref).abs()
        assert (err <= exact_ints.bf16_half_ulp(ref)).all(), err.max()


@requires_gpu
@pytest.mark.parametrize("B,K,N,wgrad", [
    (65 * BK, 432, 1024, "wgrad_nt256"),  # a last batch: short last slab
    (65 * BK, 512, 256, "wgrad_nt128"),   # N*K = 256*512: the 128 side
    (65 * BK + 4, 432, 1024, None),       # B % 64 != 0: library wgrad
])
def test_linear_bias_relu_default_routing_model_layers(B, K, N, wgrad):
    """The model's layer shapes at a ragged batch, through autograd: the
    routing must pick the kernel named here, and what it returns as dw is
    that kernel's exact, once-rounded result."""
    gen = _gen(B + K + N)
    exact_ints.assert_exact(1, 1, K, extra=2)
    exact_ints.assert_exact(2, 1, max(B, N))
    x = exact_ints.ints((B, K), 1, gen)
    w = exact_ints.ints((N, K), 1, gen)
    bias = exact_ints.ints((N,), 2, gen)
    g = exact_ints.ints((B, N), 2, gen)

    z = x.double() @ w.double().t() + bias.double()
    # the backward's mask is y > 0 on the bf16 y; RNE keeps the sign
    mask = (z > 0).double()
    dz = g.double() * mask
    ref_dw, ref_dx, ref_db = dz.t() @ x.double(), dz @ w.double(), dz.sum(0)

    xg, wg, bg = (_dev(t, BF16).requires_grad_(True) for t in (x, w, bias))
    picked = ops._custom_wgrad_kernel(_dev(g, BF16), xg.detach())
    assert picked is (getattr(ops._C, wgrad) if wgrad else None)
    y = ops.linear_bias_relu(xg, wg, bg)
    y.backward(_dev(g, BF16))

    assert torch.equal(y.detach().cpu(), exact_ints.rne_bf16(torch.relu(z)))
    assert torch.equal(bg.grad.cpu(), exact_ints.rne_bf16(ref_db))
    if wgrad:
        assert torch.equal(wg.grad.cpu(), exact_ints.rne_bf16(ref_dw))
    for got, ref in ((xg.grad, ref_dx), (wg.grad, ref_dw)):
        err = (got.double().cpu() - ref).abs()
        assert (err <= exact_ints.bf16_half_ulp(ref)).all(), err.max()


# ---- 4. bias+ReLU epilogues -------------------------------------------------

# (rows, cols, dtype): the branch each shape is there for
_DB_SHAPES = [
    (1, 8, F32), (5, 516, F32),     # row tail (rows % 4 != 0), one block
    (1023, 516, F32),
    (8192 + 7, 8, F32),             # > 4*2048 rows: quad kernel wraps + tail
    (33, 1028, F32), (9, 8192, F32),  # quads > blockDim: the k > 0 loop,
                                      # 8192 = last legal width; S <= 64 and
                                      # cols >= 1024: reduce_splitk's kernel
    (1, 8, BF16), (5, 516, BF16), (1023, 516, BF16),  # bf16 quad kernel
    (33, 1028, BF16), (9, 8192, BF16),
    (32768 + 40, 256, BF16),        # oct kernel, rpb = 8, grid wraps
    (37, 512, BF16),                # oct kernel, rpb = 4
    (70, 1024, BF16), (70, 2048, BF16),  # oct kernel, rpb = 1
    (50, 432, BF16),                # octs = 54 does not divide 256: quad
    (8192 + 7, 8, BF16),            # oct kernel with 256 one-oct slots
]


def _epilogue_data(rows, cols, seed):
    gen = _gen(seed)
    exact_ints.assert_exact(2, 1, rows)  # column sums of dy stay exact
    dy = exact_ints.ints((rows, cols), 2, gen)
    x = exact_ints.ints((rows, cols), 3, gen)
    bias = exact_ints.ints((cols,), 2, gen)
    return dy, x, bias


@requires_gpu
@pytest.mark.parametrize("rows,cols,dtype", _DB_SHAPES)
def test_bias_relu_bwd_db_exact(rows, cols, dtype):
    dy, x, bias = _epilogue_data(rows, cols, rows + cols)
    y = torch.relu(x + bias)
    ref_dx = (dy * (y > 0)).double()
    ref_db = ref_dx.sum(0)
    modes = (False, True) if dtype == BF16 else (False,)
    for dbias_bf16 in modes:
        dx, db = ops._C.bias_relu_bwd_db(_dev(dy, dtype), _dev(y, dtype),
                                         dbias_bf16)
        assert dx.dtype == dtype
        assert torch.equal(dx.double().cpu(), ref_dx)
        if dbias_bf16:
            assert torch.equal(db.cpu(), exact_ints.rne_bf16(ref_db))
        else:
            assert db.dtype == F32
            assert torch.equal(db.cpu(), ref_db.float())


@requires_gpu
@pytest.mark.parametrize("rows,cols,dtype", _DB_SHAPES + [
    (5, 7, F32), (5, 7, BF16), (3, 1, F32),   # cols % 4 != 0: scalar kernels
    (1023, 516 + 2, BF16),
    (8192 + 7, 516, F32),                     # > 2048*256 quads: fwd wraps
])
def test_bias_relu_fwd_bwd_exact(rows, cols, dtype):
    dy, x, bias = _epilogue_data(rows, cols, rows + cols)
    ref_y = torch.relu(x + bias)
    y = ops.bias_relu_fwd(_dev(x, dtype), _dev(bias, dtype))
    assert y.dtype == dtype
    assert torch.equal(y.double().cpu(), ref_y.double())
    dx = ops.bias_relu_bwd(_dev(dy, dtype), y)
    assert torch.equal(dx.double().cpu(), (dy * (ref_y > 0)).double())


# ---- 5. col_reduce_dot, row_dot, reduce_splitk ------------------------------

@requires_gpu
@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("rows,cols", [
    (3, 4),             # one quad, 3 of a block's 4 rows
    (10001, 256),       # multi-slot map (4 slots), rows % 4 != 0
    (37, 432),          # quads = 108 does not divide 256: 1D map, block 128
    (37, 768),          # quads = 192: 1D map, block 256
    (21, 1028),         # quads = 257 > blockDim: the k > 0 loop
    (9, 8192),          # last legal width, k up to 7
    (8192 + 5, 1028),   # > 4*2048 rows: the 1D map's grid wraps, with tail
])
def test_col_reduce_dot_exact(rows, cols, dtype):
    x, dy = exact_ints.operands((rows, cols), (rows,), rows,
                                seed=rows + cols)
    out = ops.col_reduce_dot(_dev(x, dtype), _dev(dy, dtype))
    ref = (x.double() * dy.double().unsqueeze(1)).sum(0)
    assert out.dtype == F32 and out.shape == (cols,)
    assert torch.equal(out.cpu(), ref.float())


@requires_gpu
@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("rows,cols", [
    (32768 + 21, 4), (32768 + 21, 12),    # > 2048*16 row groups: wraps;
    (32768 + 21, 64), (32768 + 21, 512),  # 1, 3, 16, 128 quads per row
    (1, 64), (3, 12),                     # a partly idle wave
])
def test_row_dot_exact(rows, cols, with_bias, dtype):
    # +-8 weights so the 512-wide sums pass 256 and bf16 really rounds
    x, w = exact_ints.operands((rows, cols), (cols,), cols, amax_b=8,
                               extra=5, seed=rows + cols)
    bias = torch.tensor([5], dtype=torch.int16)
    ref = x.double() @ w.double()
    if with_bias:
        ref = ref + 5.0
    out = ops._C.row_dot(_dev(x, dtype), _dev(w, dtype),
                         _dev(bias, dtype) if with_bias else None)
    assert out.shape == (rows,) and out.dtype == dtype
    if dtype == BF16:
        assert torch.equal(out.cpu(), exact_ints.rne_bf16(ref))
    else:
        assert torch.equal(out.cpu(), ref.float())


@requires_gpu
@pytest.mark.parametrize("out_bf16", [False, True])
@pytest.mark.parametrize("S,nm", [
    (1, 1024),                  # own kernel, nothing to add
    (64, 1024),                 # own kernel: last S and first nm it takes
    (65, 1024),                 # S > 64: torch.sum
    (3, 512),                   # nm < 1024: torch.sum
    (2, 4 * (524288 + 37)),     # own kernel, > 2048*256 quads: grid wraps
])
def test_reduce_splitk_exact(S, nm, out_bf16):
    exact_ints.assert_exact(256, 1, S)
    part = exact_ints.ints((S, nm), 256, _gen(S + nm))
    out = ops._C.reduce_splitk(_dev(part, F32), out_bf16)
    ref = part.double().sum(0)
    assert out.shape == (nm,)
    if out_bf16:
        assert torch.equal(out.cpu(), exact_ints.rne_bf16(ref))
    else:
        assert out.dtype == F32
        assert torch.equal(out.cpu(), ref.float())


# ---- 6. fused BCE head ------------------------------------------------------

_BCE_N = 256 * 2048 + 5   # 5 past a full grid: the grid-stride loop wraps


def _bce_inputs():
    """Three bf16 logit parts whose fp32 sum, in the kernel's order
    (deep + wide) + dhead, is exact: all are multiples of 2**-6 below
    2**7.  z = deep + s*d/4 covers [-64, 64] in steps of 1/4, and [-4, 4]
    in steps of 1/64, while for s != 0 wide = +-64 and dhead = -+(64 - d/4)
    cancel to a small remainder."""
    gen = _gen(60)
    n = _BCE_N
    a = torch.randint(-240, 241, (n,), generator=gen).double()
    fine = torch.rand(n, generator=gen) < 0.3
    deep = torch.where(fine, a / 64, a / 4)
    s = torch.randint(-1, 2, (n,), generator=gen).double()
    d = torch.randint(0, 17, (n,), generator=gen).double()
    wide = s * 64
    dhead = torch.where(s == 0, d / 4 - 2, -s * (64 - d / 4))
    parts = [deep, wide, dhead]
    for p in parts:
        assert torch.equal(p.to(BF16).double(), p)   # bf16 holds each part
    z = (deep + wide) + dhead
    assert torch.equal(z.float().double(), z)
    assert z.min() <= -60 and z.max() >= 60
    labels = (torch.rand(n, generator=gen) > 0.5).double()
    return parts, z, labels


@requires_gpu
def test_bce_head_loss_per_element():
    parts, z, labels = _bce_inputs()
    loss = ops.BCEHeadFn.apply(*[_dev(p, BF16) for p in parts],
                               _dev(labels, F32))
    assert loss.dtype == F32 and loss.shape == (_BCE_N,)
    soft = torch.log1p(torch.exp(-z.abs()))          # in (0, ln 2]
    ref = torch.clamp(z, min=0) - z * labels + soft
    # max(z,0) - z*y is exact in fp32 (y is 0 or 1).  expf and log1pf are
    # documented to 1 ulp each in the ROCm device library; an input error
    # of 1 ulp in e moves log1p(e) by e/(1+e) <= log1p(e) ulps, so the soft
    # term carries at most 2 ulps of itself (4 allowed), near 0 included
    # since the bound is relative to the term.  The final add rounds once:
    # half an ulp of the result (1 allowed).
    ulp = 2.0 ** -23
    tol = 4 * ulp * soft + ulp * ref.abs()
    err = (loss.double().cpu() - ref).abs()
    worst = (err / tol).max().item()
    assert (err <= tol).all(), f"worst err/tol {worst}"


@requires_gpu
@pytest.mark.parametrize("upstream", ["sum", "pow2", "mean"])
def test_bce_head_gradient_scale_aware(upstream):
    parts, z, labels = _bce_inputs()
    dev_parts = [_dev(p, BF16).requires_grad_(True) for p in parts]
    loss = ops.BCEHeadFn.apply(*dev_parts, _dev(labels, F32))
    if upstream == "sum":
        g = torch.ones(_BCE_N, dtype=torch.float64)
        loss.sum().backward()
    elif upstream == "pow2":
        # a different g per element, of order 1: +-2**k, k in [-2, 2].
        # Powers of two because the bound below needs them: scaling by
        # one moves (sigmoid - y) to another binade unchanged, so the
        # result's half-ulp stays 2**-9 * |g|; for a general g it is up
        # to 2**-8 * |g| and correct arithmetic would miss the bound.
        gen = _gen(61)
        k = torch.randint(-2, 3, (_BCE_N,), generator=gen)
        sign = torch.randint(0, 2, (_BCE_N,), generator=gen) * 2 - 1
        g32 = torch.ldexp(sign.float(), k)
        g = g32.double()
        loss.backward(g32.cuda())
    else:
        # the fp32 1/n that mean()'s backward hands down
        g = torch.full((_BCE_N,), 1.0, dtype=torch.float32) / _BCE_N
        g = g.double()
        loss.mean().backward()
    ref = (torch.sigmoid(z) - labels) * g
    # dl = bf16((bf16(sigmoid) - y) * g): half a bf16 ulp of the saved
    # sigmoid (<= 1, so 2**-9) times |g|, plus half a bf16 ulp of the
    # result: |sigmoid - y| < 1, so the result lies below |g| rounded up
    # to a power of two, p, and its half-ulp is at most 2**-9 * p.  For
    # sum and pow2 p = |g|: the bound is (2**-9 + 2**-9) * |g|.  mean()'s
    # 1/n sits 1e-5 below 2**-19 = p, so it is held to 2**-8 / n (1 +
    # 5e-6), relative to 1/n and not to an absolute number.
    mant, expo = torch.frexp(g.abs())
    p = torch.where(mant == 0.5, g.abs(),
                    torch.ldexp(torch.ones_like(g), expo))
    bound = 2.0 ** -9 * g.abs() + 2.0 ** -9 * p
    if upstream != "mean":
        assert torch.equal(bound, (2.0 ** -9 + 2.0 ** -9) * g.abs())
    for p in dev_parts:
        dl = p.grad.double().cpu()
        assert (dl - ref).abs().le(bound).all(), \
            ((dl - ref).abs() / g.abs()).max().item()
        sure = ref.abs() > bound
        assert sure.sum() > _BCE_N // 4
        assert torch.equal(torch.sign(dl[sure]), torch.sign(ref[sure]))
