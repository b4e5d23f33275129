#!/usr/bin/env python3
"""Micro-benchmark of the multi-hot embedding-bag kernels at the bench
shape (b=65536, 26 features x 1M rows, dim 16, bf16 out into the 432-column
MLP-input buffer behind its 16 dense/pad columns).

Three laws for the bag lengths:
  len1      every bag holds one id (the one-hot data as bags);
  uniform8  lengths uniform in 1..8;
  zipf256   P(len = l) ~ l^-1.5 for l in 1..256.

Timed for each law:
  (a) emb_bag_fwd from the raw ids + per-feature offsets, per combiner;
  (b) emb_bag_bwd_rows on the strided gradient slice ("mean");
  (c) the torch composition (a) replaces: F.embedding_bag in fp32 (from
      PRE-ADDED flat ids, which torch needs and is not charged for), the
      cast to bf16 and the copy into the slice; "sqrtn" as a "sum" scaled
      by a precomputed 1/sqrt(len);
  (d) len1 only: emb_fwd_into on the same (pre-added) ids.

Each figure is the median over --repeats windows of --iters calls (device
events around each window, after a warm-up window), with min..max as the
spread.  Calls rotate over --sets independent input sets, so inputs come
from HBM and not from a cache the previous call warmed.  Next to each time
the script prints the bytes the call must move, counted from the shapes
(every table row read counted once per entry, no reuse assumed), and the
resulting TB/s.  --json PATH also writes the numbers to a file."""

import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F_

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tf_yarn_amd import ops  # noqa: E402

F = 26
DIM = 16
PAD = 16
COMBINERS = ("sum", "mean", "sqrtn")


def timed(fn, iters, repeats):
    """us per call: (median, min, max) over `repeats` event-timed windows;
    fn(i) gets the call number so it can rotate its inputs."""
    for i in range(iters):
        fn(i)
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        t0 = torch.cuda.Event(enable_timing=True)
        t1 = torch.cuda.Event(enable_timing=True)
        t0.record()
        for i in range(iters):
            fn(i)
        t1.record()
        torch.cuda.synchronize()
        out.append(t0.elapsed_time(t1) * 1e3 / iters)
    return statistics.median(out), min(out), max(out)


def draw_lengths(law, n_bags, gen):
    if law == "len1":
        return torch.ones(n_bags, dtype=torch.int64, device="cuda")
    if law == "uniform8":
        return torch.randint(1, 9, (n_bags,), device="cuda", generator=gen)
    p = torch.arange(1, 257, device="cuda", dtype=torch.float64) ** -1.5
    return torch.multinomial(p, n_bags, replacement=True, generator=gen) + 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--rows-per-table", type=int, default=1_000_000)
    ap.add_argument("--sets", type=int, default=6)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--laws", default="len1,uniform8,zipf256")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    B, S, R = args.batch, args.sets, args.rows_per_table
    n_bags = B * F
    cols = PAD + F * DIM
    bf16 = torch.bfloat16
    gen = torch.Generator(device="cuda").manual_seed(0)

    table = torch.randn(R * F, DIM, device="cuda")
    offsets = torch.arange(F, device="cuda") * R
    out = [torch.empty(B, cols, dtype=bf16, device="cuda") for _ in range(S)]
    gbuf = [torch.randn(B, cols, device="cuda").to(bf16) for _ in range(S)]

    res = {"batch": B, "rows": R * F, "sets": S, "iters": args.iters,
           "repeats": args.repeats}

    def record(name, fn, nbytes):
        med, lo, hi = timed(fn, args.iters, args.repeats)
        res[name] = {"median_us": round(med, 1), "min_us": round(lo, 1),
                     "max_us": round(hi, 1), "bytes": int(nbytes),
                     "tb_per_s": round(nbytes / med / 1e6, 3)}
        print(f"{name:34s} {med:9.1f} us  ({lo:.1f} .. {hi:.1f})  "
              f"{nbytes / 1e6:9.1f} MB  {nbytes / med / 1e6:6.3f} TB/s",
              flush=True)

    for law in args.laws.split(","):
        ids, flat, bos, scales, rsq = [], [], [], [], []
        for _ in range(S):
            lens = draw_lengths(law, n_bags, gen)
            bo = torch.zeros(n_bags + 1, dtype=torch.int64, device="cuda")
            bo[1:] = torch.cumsum(lens, 0)
            nnz = int(bo[-1])
            raw = torch.randint(0, R, (nnz,), device="cuda", generator=gen)
            feat = torch.arange(n_bags, device="cuda") % F
            ids.append(raw)
            flat.append(raw + torch.repeat_interleave(offsets[feat], lens))
            bos.append(bo)
            scales.append(1.0 / lens.float())
            rsq.append((1.0 / lens.float().sqrt()).unsqueeze(1))
        nnz = sum(i.numel() for i in ids) / S  # mean over the sets
        res[law] = {"mean_nnz": nnz, "mean_len": nnz / n_bags}
        print(f"--- {law}: mean nnz {nnz:.0f} ({nnz / n_bags:.2f} per bag)",
              flush=True)
        offs_b = (n_bags + 1) * 8
        fwd_b = (nnz * 8 + offs_b + nnz * DIM * 4 + n_bags * DIM * 2
                 + n_bags * 4 + nnz * 8)
        bwd_b = n_bags * DIM * 2 + offs_b + n_bags * 4 + nnz * DIM * 2
        # torch: ids + offsets + rows, fp32 result out and back in for the
        # cast, bf16 out and back in for the copy, the slice
        torch_b = (nnz * 8 + offs_b + nnz * DIM * 4
                   + 2 * n_bags * DIM * 4 + 3 * n_bags * DIM * 2)

        for comb in COMBINERS:
            record(f"{law}_a_emb_bag_fwd_{comb}",
                   lambda i, c=comb: ops.emb_bag_fwd(
                       table, ids[i % S], bos[i % S], F, offsets=offsets,
                       combiner=c, out=out[i % S], col_offset=PAD), fwd_b)
        record(f"{law}_b_emb_bag_bwd_rows_mean",
               lambda i: ops.emb_bag_bwd_rows(
                   gbuf[i % S], bos[i % S], scales[i % S], DIM, F,
                   col_offset=PAD, nnz=ids[i % S].numel()), bwd_b)

        def torch_comp(i, comb):
            k = i % S
            pooled = F_.embedding_bag(
                flat[k], table, bos[k][:-1],
                mode="sum" if comb == "sqrtn" else comb)
            if comb == "sqrtn":
                pooled = pooled * rsq[k]
            out[k][:, PAD:] = pooled.to(bf16).reshape(B, F * DIM)

        for comb in COMBINERS:
            extra = 2 * n_bags * DIM * 4 if comb == "sqrtn" else 0
            record(f"{law}_c_torch_embedding_bag_{comb}",
                   lambda i, c=comb: torch_comp(i, c), torch_b + extra)
        if law == "len1":
            record("len1_d_emb_fwd_into",
                   lambda i: ops.emb_fwd_into(table, flat[i % S], out[i % S],
                                              PAD),
                   nnz * 8 + nnz * DIM * 4 + nnz * DIM * 2)
        del ids, flat, bos, scales, rsq

    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)),
                    exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
