"""References and input builders shared by the embedding-bag tests.

The definition under test (``tf_yarn_amd.ops.emb_bag_fwd``): bag
``k = b*F + f`` holds entries ``bag_offsets[k] .. bag_offsets[k+1]-1``;
entry ``i`` names row ``ids[i] + offsets[k % F]``; per bag and column
``out = (sum_i w_i * row_i) * bag_scale[k]`` with ``bag_scale`` 1 ("sum"),
``1/sum w`` ("mean") or ``1/sqrt(sum w^2)`` ("sqrtn"), ``w_i = 1`` without
weights, and 0 for an empty bag or a zero denominator.

Everything here runs on the CPU in float64.
"""

import math

import torch

COMBINERS = ("sum", "mean", "sqrtn")


def make_bags(lengths, sizes, gen, id_lo=0):
    """Raw per-feature ids for bags of the given lengths (bag ``k`` is
    feature ``k % len(sizes)``): ``(ids [nnz], bag_offsets [n_bags + 1],
    offsets [F])``.  ``id_lo``: the smallest raw id drawn."""
    lengths = torch.as_tensor(lengths, dtype=torch.int64)
    n_features = len(sizes)
    assert lengths.numel() % n_features == 0
    bag_offsets = torch.zeros(lengths.numel() + 1, dtype=torch.int64)
    bag_offsets[1:] = torch.cumsum(lengths, 0)
    sizes_t = torch.tensor(sizes, dtype=torch.int64)
    feat = torch.arange(lengths.numel()) % n_features
    hi = torch.repeat_interleave(sizes_t[feat], lengths)
    nnz = int(bag_offsets[-1])
    u = torch.rand(nnz, generator=gen, dtype=torch.float64)
    ids = id_lo + (u * (hi - id_lo).double()).long()
    ids = torch.minimum(ids, hi - 1)
    offsets = torch.zeros(n_features, dtype=torch.int64)
    offsets[1:] = torch.cumsum(sizes_t, 0)[:-1]
    return ids, bag_offsets, offsets


def bag_of_entry(bag_offsets):
    lens = bag_offsets[1:] - bag_offsets[:-1]
    return torch.repeat_interleave(torch.arange(lens.numel()), lens)


def flat_ids_of(ids, bag_offsets, offsets):
    n_features = offsets.numel()
    return ids + offsets[bag_of_entry(bag_offsets) % n_features]


def loop_ref64(table, ids, bag_offsets, n_features, offsets=None,
               weights=None, combiner="sum"):
    """A plain Python loop over bags, float64: ``(acc64 [n_bags, dim],
    scale64 [n_bags])``; the pooled value is ``acc64 * scale64``."""
    bo = bag_offsets.tolist()
    n_bags = len(bo) - 1
    t64 = table.double()
    acc = torch.zeros(n_bags, table.shape[1], dtype=torch.float64)
    scale = torch.zeros(n_bags, dtype=torch.float64)
    for k in range(n_bags):
        off = int(offsets[k % n_features]) if offsets is not None else 0
        den = 0.0
        for i in range(bo[k], bo[k + 1]):
            w = float(weights[i]) if weights is not None else 1.0
            acc[k] += w * t64[int(ids[i]) + off]
            den += w * w if combiner == "sqrtn" else w
        if bo[k + 1] > bo[k]:
            if combiner == "sum":
                scale[k] = 1.0
            elif den != 0.0:
                scale[k] = 1.0 / (math.sqrt(den) if combiner == "sqrtn"
                                  else den)
    return acc, scale


def segment_ref64(table, flat_ids, bag_offsets, weights=None,
                  combiner="sum"):
    """The same in one float64 ``index_add_`` (any order: for operands
    whose sums are exact), for cases with too many bags to loop over."""
    n_bags = bag_offsets.numel() - 1
    bag = bag_of_entry(bag_offsets)
    w = (weights.double() if weights is not None
         else torch.ones(flat_ids.numel(), dtype=torch.float64))
    acc = torch.zeros(n_bags, table.shape[1], dtype=torch.float64)
    acc.index_add_(0, bag, w.unsqueeze(1) * table.double()[flat_ids])
    den = torch.zeros(n_bags, dtype=torch.float64)
    den.index_add_(0, bag, w * w if combiner == "sqrtn" else w)
    lens = bag_offsets[1:] - bag_offsets[:-1]
    if combiner == "sum":
        scale = (lens > 0).double()
    else:
        ok = (lens > 0) & (den != 0)
        d = torch.where(ok, den, torch.ones_like(den))
        if combiner == "sqrtn":
            d = d.sqrt()
        scale = torch.where(ok, 1.0 / d, torch.zeros_like(d))
    return acc, scale


def ulp32(ref64):
    """One fp32 ulp (24 significant bits) at each reference value."""
    _, exponent = torch.frexp(ref64)  # |ref| = m * 2**exponent, m in [.5, 1)
    ulp = torch.ldexp(torch.ones_like(ref64), exponent - 24)
    return torch.where(ref64 == 0, torch.zeros_like(ref64), ulp)


def assert_scale_1ulp(scale32, scale64):
    """``bag_scale`` is one correctly rounded division, or a square root
    followed by a division: within 1 ulp32 of the float64 scale."""
    err = (scale32.double() - scale64).abs()
    bad = err > ulp32(scale64)
    assert not bool(bad.any()), (
        f"bag_scale off by more than 1 ulp at bags "
        f"{torch.nonzero(bad).reshape(-1)[:8].tolist()}")


def int_model(table_sizes, dim, hidden, gen, compute_dtype=torch.float32,
              **kw):
    """A WideAndDeep whose every parameter is a small integer (weights in
    {-1, 0, 1}, biases 0, tables in [-1, 1]): with integer inputs its
    logits and, under ``logits.sum()``, every gradient are integers, exact
    in fp32 and bf16 alike."""
    from tf_yarn_amd.models.wide_deep import WideAndDeep
    model = WideAndDeep(table_sizes=table_sizes, embedding_dim=dim,
                        hidden=hidden, compute_dtype=compute_dtype, **kw)
    with torch.no_grad():
        for name, p in sorted(model.named_parameters()):
            if name.endswith("bias"):
                p.zero_()
            else:
                p.copy_(torch.randint(-1, 2, p.shape, generator=gen)
                        .to(p.dtype))
    return model
