"""The embedding-bag HIP kernels at the shapes where they can go wrong.

Operands are integers (``exact_ints``): table values in [-8, 8], weights
in [-4, 4], bags of at most 300 entries, so the worst partial sum is
``8 * 4 * 300 = 9600 < 2**24`` and ``acc`` is exact in any order: it
equals the float64 sum.  What is left is the scale: the returned
``bag_scale`` must sit within 1 ulp32 of the float64 one (one correctly
rounded division, or a square root followed by a division), and ``out``
must be ``acc * bag_scale`` computed by torch in fp32 from the RETURNED
scale, rounded once for bf16.  That separates the sum and the placement
from the rounding of the scale; there is no tolerance to pick.  The
backward is products only (nothing to contract), compared with
``torch.equal`` against torch's own fp32 products."""

import copy
import functools

import pytest
import torch

import emb_bag_ref as R
import exact_ints
from tf_yarn_amd import ops

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X"),
]

TABLE_AMAX, WEIGHT_AMAX, MAX_LEN = 8, 4, 300
SENTINEL = -77.0


def _lengths(n, lo, hi, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, (n,), generator=g)


def _edges(n):
    """First, a middle and the last bag empty."""
    lens = _lengths(n, 1, 4, 11)
    lens[0] = lens[n // 2] = lens[-1] = 0
    return lens


def _long():
    lens = _lengths(6, 0, 3, 12)
    lens[1] = MAX_LEN
    return lens


# name -> (B, F, dim, col_offset, spare columns behind, rows per feature,
#          lengths)
CASES = {
    "b1_f1": (1, 1, 16, 0, 0, 5, torch.tensor([1])),
    "model_layout": (5, 26, 16, 16, 0, 11, _lengths(5 * 26, 0, 9, 1)),
    "empty_edges": (3, 3, 16, 16, 4, 9, _edges(9)),
    "all_empty": (2, 3, 16, 4, 4, 9, torch.zeros(6, dtype=torch.int64)),
    "long_bag": (2, 3, 16, 0, 0, 40, _long()),
    "dim4": (3, 4, 4, 4, 4, 9, _lengths(12, 0, 5, 2)),
    "dim64": (3, 4, 64, 16, 0, 9, _lengths(12, 0, 5, 3)),
    "dim12": (3, 4, 12, 8, 4, 9, _lengths(12, 0, 5, 4)),
    "dim1_scalar": (7, 5, 1, 2, 3, 9, _lengths(35, 0, 5, 5)),
    "dim7_scalar": (3, 4, 7, 5, 2, 9, _lengths(12, 0, 5, 6)),
    "dim16_col3_scalar": (3, 4, 16, 3, 1, 9, _lengths(12, 0, 5, 7)),
    "untouched_cols": (4, 3, 16, 16, 8, 9, _lengths(12, 0, 4, 8)),
    "repeated_ids": (6, 4, 16, 0, 0, 3, _lengths(24, 0, 6, 9)),
    # 2048 blocks x 256 threads own one (bag, quad) each per trip at dim 4:
    # 37 threads take a second grid-stride trip
    "grid_wrap": ((2048 * 256 + 37) // 3, 3, 4, 0, 0, 50,
                  _lengths(2048 * 256 + 37, 0, 2, 10)),
}
ZERO_DEN_BAG = 1  # of "model_layout": weights +1, -1


@functools.lru_cache(maxsize=None)
def _inputs(case, weighted):
    """Inputs of a case and its float64 reference per combiner, built once
    and shared (never modified) by every test of the case."""
    b, f, dim, col, spare, rows, lengths = CASES[case]
    assert lengths.numel() == b * f and int(lengths.max()) <= MAX_LEN
    exact_ints.assert_exact(TABLE_AMAX, WEIGHT_AMAX, MAX_LEN)
    g = torch.Generator().manual_seed(100 + len(case))
    if case == "model_layout":
        lengths = lengths.clone()
        lengths[ZERO_DEN_BAG] = 2
    ids, bo, offsets = R.make_bags(lengths, [rows] * f, g)
    table = exact_ints.ints((rows * f, dim), TABLE_AMAX, g).float()
    w = None
    if weighted:
        w = torch.randint(-WEIGHT_AMAX, WEIGHT_AMAX + 1, (ids.numel(),),
                          generator=g).float()
        if case == "model_layout":
            w[bo[ZERO_DEN_BAG]:bo[ZERO_DEN_BAG] + 2] = \
                torch.tensor([1.0, -1.0])
    flat = R.flat_ids_of(ids, bo, offsets)
    refs = {c: R.segment_ref64(table, flat, bo, w, c) for c in R.COMBINERS}
    return dict(table=table, ids=ids, bo=bo, offsets=offsets, flat=flat,
                w=w, refs=refs, bag=R.bag_of_entry(bo))


def _cuda(t):
    return None if t is None else t.cuda()


def _expected_block(acc64, scale32, batch, dtype):
    return (acc64.float() * scale32.unsqueeze(1)).reshape(batch, -1) \
        .to(dtype)


@pytest.mark.parametrize("weighted", [False, True],
                         ids=["noweights", "weights"])
@pytest.mark.parametrize("raw_ids", [True, False], ids=["raw+offsets", "flat"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16],
                         ids=["f32", "bf16"])
@pytest.mark.parametrize("case", list(CASES))
def test_forward(case, dtype, raw_ids, weighted):
    b, f, dim, col, spare, _, _ = CASES[case]
    inp = _inputs(case, weighted)
    table, bo, w, flat = inp["table"], inp["bo"], inp["w"], inp["flat"]
    ids, offsets = (inp["ids"], inp["offsets"]) if raw_ids else (flat, None)
    cols = col + f * dim + spare
    table_g, ids_g, bo_g = table.cuda(), ids.cuda(), bo.cuda()
    for combiner in R.COMBINERS:
        acc, scale64 = inp["refs"][combiner]
        out = torch.full((b, cols), SENTINEL, dtype=dtype, device="cuda")
        got, scale, fl = ops.emb_bag_fwd(
            table_g, ids_g, bo_g, f, offsets=_cuda(offsets),
            weights=_cuda(w), combiner=combiner, out=out, col_offset=col)
        assert got is out
        out_c, scale_c = out.cpu(), scale.cpu()
        block = out_c[:, col:col + f * dim]
        R.assert_scale_1ulp(scale_c, scale64)
        assert torch.equal(block,
                           _expected_block(acc, scale_c, b, dtype)), combiner
        if combiner == "sum":
            want = acc.reshape(b, -1)
            if dtype == torch.bfloat16:
                want = exact_ints.rne_bf16(want).double()
            assert torch.equal(block.double(), want)
        assert bool((out_c[:, :col] == SENTINEL).all())
        assert bool((out_c[:, col + f * dim:] == SENTINEL).all())
        assert torch.equal(fl.cpu(), flat)
        if not raw_ids:
            assert fl.data_ptr() == ids_g.data_ptr()
        if case == "model_layout" and weighted and combiner == "mean":
            assert scale_c[ZERO_DEN_BAG] == 0
            assert not block.reshape(-1, dim)[ZERO_DEN_BAG].any()
        # the CPU path of the same call
        out_cpu = torch.full((b, cols), SENTINEL, dtype=dtype)
        _, scale_cpu, fl_cpu = ops.emb_bag_fwd(
            table, ids, bo, f, offsets=offsets, weights=w,
            combiner=combiner, out=out_cpu, col_offset=col)
        assert torch.equal(fl_cpu, flat)
        assert bool(((scale_c.double() - scale_cpu.double()).abs()
                     <= R.ulp32(scale_cpu.double())).all())
        if torch.equal(scale_c, scale_cpu):
            assert torch.equal(out_c, out_cpu), combiner
        else:  # the scales may differ by their 1 ulp; the sums may not
            assert torch.equal(out_cpu[:, col:col + f * dim],
                               _expected_block(acc, scale_cpu, b, dtype))


@pytest.mark.parametrize("weighted", [False, True],
                         ids=["noweights", "weights"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16],
                         ids=["f32", "bf16"])
@pytest.mark.parametrize("case", list(CASES))
def test_backward_rows(case, dtype, weighted):
    b, f, dim, col, spare, _, _ = CASES[case]
    inp = _inputs(case, weighted)
    bo, w, bag = inp["bo"], inp["w"], inp["bag"]
    nnz = inp["ids"].numel()
    cols = col + f * dim + spare
    g = torch.Generator().manual_seed(7)
    # the gradient is a column slice of a wider buffer, read in place
    wider = torch.randn(b, cols + 8, generator=g).to(dtype)
    grad = wider[:, :cols]
    grad_g = wider.cuda()[:, :cols]
    assert b == 1 or grad_g.stride(0) == cols + 8
    rows_of = grad[:, col:col + f * dim].reshape(b * f, dim)[bag]
    bo_g = bo.cuda()
    for combiner in R.COMBINERS:
        scale = inp["refs"][combiner][1].float()
        rows = ops.emb_bag_bwd_rows(grad_g, bo_g, scale.cuda(), dim, f,
                                    weights=_cuda(w), col_offset=col)
        assert rows.dtype == dtype and rows.shape == (nnz, dim)
        if combiner == "sum" and not weighted:
            assert torch.equal(rows.cpu(), rows_of)
            continue
        s = scale[bag] * w if weighted else scale[bag]
        want = (rows_of.float() * s.unsqueeze(1)).to(dtype)
        assert torch.equal(rows.cpu(), want), combiner


def test_fractional_weights_match_the_cpu_path():
    """Random fp32 tables and weights: the sequential fmaf sum, the
    unfused ``w * w`` denominator and the correctly rounded sqrt and
    division give the CPU path's bits."""
    g = torch.Generator().manual_seed(21)
    f, dim, rows = 4, 16, 30
    lengths = _lengths(5 * f, 0, 12, 22)
    ids, bo, offsets = R.make_bags(lengths, [rows] * f, g)
    table = torch.randn(rows * f, dim, generator=g)
    w = torch.rand(ids.numel(), generator=g) + 0.25
    for combiner in R.COMBINERS:
        for weights in (None, w):
            out, scale, _ = ops.emb_bag_fwd(
                table.cuda(), ids.cuda(), bo.cuda(), f,
                offsets=offsets.cuda(), weights=_cuda(weights),
                combiner=combiner)
            out_cpu, scale_cpu, _ = ops.emb_bag_fwd(
                table, ids, bo, f, offsets=offsets, weights=weights,
                combiner=combiner)
            assert torch.equal(scale.cpu(), scale_cpu), combiner
            assert torch.equal(out.cpu(), out_cpu), combiner


def test_host_checks_raise_before_any_launch():
    inp = _inputs("dim4", True)
    b, f, dim, col, spare, _, _ = CASES["dim4"]
    table, ids, bo = inp["table"].cuda(), inp["ids"].cuda(), inp["bo"].cuda()
    offsets, w = inp["offsets"].cuda(), inp["w"].cuda()
    with pytest.raises(ValueError, match="bag_offsets"):
        ops.emb_bag_fwd(table, ids, bo[:-1].contiguous(), f, offsets=offsets)
    with pytest.raises(ValueError, match="weights"):
        ops.emb_bag_fwd(table, ids, bo, f, offsets=offsets, weights=w[:-1])
    with pytest.raises(ValueError, match="combiner"):
        ops.emb_bag_fwd(table, ids, bo, f, offsets=offsets, combiner="max")
    with pytest.raises(RuntimeError, match="combiner"):
        ops._C.emb_bag_fwd(table, ids, bo, f, offsets, None, "max",
                           torch.empty(b, f * dim, device="cuda"), 0)
    with pytest.raises(RuntimeError, match="bag_offsets"):
        ops._C.emb_bag_fwd(table, ids, bo[:-1].contiguous(), f, offsets,
                           None, "sum",
                           torch.empty(b, f * dim, device="cuda"), 0)
    with pytest.raises(RuntimeError, match="weights"):
        ops._C.emb_bag_fwd(table, ids, bo, f, offsets, w[:-1].contiguous(),
                           "sum", torch.empty(b, f * dim, device="cuda"), 0)
    with pytest.raises(RuntimeError, match="slice out of range"):
        ops._C.emb_bag_fwd(table, ids, bo, f, offsets, None, "sum",
                           torch.empty(b, f * dim, device="cuda"), 4)
    with pytest.raises(RuntimeError, match="int64"):
        ops._C.emb_bag_fwd(table, ids.int(), bo, f, offsets, None, "sum",
                           torch.empty(b, f * dim, device="cuda"), 0)


# ---- the model -------------------------------------------------------------

MODEL_SIZES = [7, 5, 6]
MODEL_LR = 1.0


def _close(gpu, cpu):  # tests/test_sparse_ftrl_gpu.py's, for its model cases
    return torch.allclose(gpu.cpu(), cpu, atol=1e-5)


@pytest.mark.parametrize("rules", [
    dict(sparse_optimizer="sgd"),
    dict(sparse_optimizer="adagrad", wide_sparse_optimizer="ftrl",
         sparse_initial_accumulator=0.1),
], ids=["sgd", "adagrad+ftrl"])
def test_wide_and_deep_two_steps_match_the_cpu_path(rules):
    """Integer parameters and inputs and ``logits.sum()`` as the loss:
    activations, logits and every gradient are integers, exact in bf16 on
    both sides, so under SGD with lr 1 the tables stay integers and must
    be equal bit for bit."""
    g = torch.Generator().manual_seed(31)
    cpu = R.int_model(MODEL_SIZES, 4, (4,), g,
                      compute_dtype=torch.bfloat16, **rules)
    gpu = copy.deepcopy(cpu).cuda()
    nf = len(MODEL_SIZES)
    sgd = rules["sparse_optimizer"] == "sgd"
    for step in range(2):
        lengths = torch.randint(0, 4, (6 * nf,), generator=g)
        ids, bo, _ = R.make_bags(lengths, MODEL_SIZES, g)
        dense = torch.randint(-1, 2, (6, 13), generator=g).float()
        w = None if sgd else \
            2.0 ** torch.randint(-1, 2, (ids.numel(),), generator=g).float()
        loss_c = cpu(dense, ids, bag_offsets=bo, sparse_weights=w) \
            .float().sum()
        loss_g = gpu(dense.cuda(), ids.cuda(), bag_offsets=bo.cuda(),
                     sparse_weights=_cuda(w)).float().sum()
        assert torch.allclose(loss_g.detach().cpu(), loss_c.detach(),
                              atol=1e-5), step
        loss_c.backward()
        loss_g.backward()
        for m in (cpu, gpu):
            (entry,) = m.deep_embedding.pending_grads()
            assert entry.grad_rows.dtype == torch.bfloat16
            assert entry.grad_rows.shape == (ids.numel(), 4)
        cpu.apply_sparse_updates(MODEL_LR)
        gpu.apply_sparse_updates(MODEL_LR)
        sd_c, sd_g = cpu.state_dict(), gpu.state_dict()
        for name, t in sd_c.items():
            if "embedding" not in name or not t.is_floating_point():
                continue
            if sgd:
                assert torch.equal(sd_g[name].cpu(), t), (step, name)
                assert torch.equal(t, t.round()), name  # still integers
            else:
                assert _close(sd_g[name], t), (step, name)
