#!/usr/bin/env python3
"""Micro-benchmark of the fused sparse forward, the head's ReLU backward
and the scatter with in-kernel offsets, at the bench shape (b=65536, 26
features x 1M rows, dim 16 deep + dim 1 wide, 13 dense features padded to
16 columns, 256-wide last hidden layer, bf16).

Timed, each fused kernel against exactly what it replaces:
  (a) offset add + emb_fwd_into + emb_gather_sum + the two fills
      against emb_lookup_fused;
  (b) the outer product dl[:, None] * w[None, :] + bias_relu_bwd_db
      against head_relu_bwd_db;
  (c) emb_bwd_sgd_fused_wide from pre-added flat ids (the offset add is
      charged to (a)) against the same kernel adding the offsets itself,
      on the model's strided gradient slice.

Each figure is the median over --repeats windows of --iters calls (device
events around each window, after a warm-up window), with min..max as the
spread.  Calls rotate over --sets independent input sets (ids, dense,
activations, gradients: ~150 MB each), so inputs come from HBM as they do
inside a training step and not from a cache the previous call warmed.
--json PATH also writes the numbers to a file."""

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tf_yarn_amd import ops  # noqa: E402

F = 26
DIM = 16
N_DENSE = 13
PAD = 16
WIDTH = 256
LR = 0.01


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--rows-per-table", type=int, default=1_000_000)
    ap.add_argument("--sets", type=int, default=6)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    C = ops._C
    B, S = args.batch, args.sets
    bf16 = torch.bfloat16

    torch.manual_seed(0)
    n_rows = args.rows_per_table * F
    table = torch.randn(n_rows, DIM, device="cuda")
    wide = torch.randn(n_rows, 1, device="cuda")
    offsets = torch.arange(F, device="cuda") * args.rows_per_table
    ids = [torch.randint(0, args.rows_per_table, (B, F), device="cuda")
           for _ in range(S)]
    flat = [(i + offsets.unsqueeze(0)).reshape(-1) for i in ids]
    dense = [torch.randn(B, N_DENSE, device="cuda").to(bf16)
             for _ in range(S)]
    out = [torch.empty(B, PAD + F * DIM, dtype=bf16, device="cuda")
           for _ in range(S)]
    # gradient of the MLP input; the scatter reads the slice in place
    gbuf = [torch.randn(B, PAD + F * DIM, device="cuda").to(bf16)
            for _ in range(S)]
    gw = [torch.randn(B, device="cuda").to(bf16) for _ in range(S)]
    y = [torch.relu(torch.randn(B, WIDTH, device="cuda")).to(bf16)
         for _ in range(S)]
    dl = [torch.randn(B, device="cuda").to(bf16) for _ in range(S)]
    w_head = (torch.randn(WIDTH, device="cuda") * 0.06).to(bf16)

    res = {"batch": B, "rows": n_rows, "sets": S, "iters": args.iters,
           "repeats": args.repeats}

    def record(name, fn):
        med, lo, hi = timed(fn, args.iters, args.repeats)
        res[name] = {"median_us": round(med, 1), "min_us": round(lo, 1),
                     "max_us": round(hi, 1)}
        print(f"{name:44s} {med:8.1f} us  ({lo:.1f} .. {hi:.1f})",
              flush=True)

    # (a) sparse forward
    def fwd_separate(i):
        k = i % S
        f = (ids[k] + offsets.unsqueeze(0)).reshape(-1)
        o = out[k]
        o[:, :N_DENSE] = dense[k]
        o[:, N_DENSE:PAD] = 0
        C.emb_fwd_into(table, f, o, PAD)
        C.emb_gather_sum(wide, f, B, True)

    def fwd_fused(i):
        k = i % S
        C.emb_lookup_fused(table, wide.reshape(-1), ids[k], offsets,
                           dense[k], out[k], PAD)

    record("a_fwd_add+into+gather_sum+fills", fwd_separate)
    record("a_fwd_emb_lookup_fused", fwd_fused)
    record("a_part_offset_add", lambda i: ids[i % S] + offsets.unsqueeze(0))
    record("a_part_emb_fwd_into",
           lambda i: C.emb_fwd_into(table, flat[i % S], out[i % S], PAD))
    record("a_part_emb_gather_sum",
           lambda i: C.emb_gather_sum(wide, flat[i % S], B, True))

    # (b) top of the MLP backward
    def head_separate(i):
        k = i % S
        C.bias_relu_bwd_db(dl[k].unsqueeze(1) * w_head.unsqueeze(0), y[k],
                           True)

    record("b_outer_product+bias_relu_bwd_db", head_separate)
    record("b_head_relu_bwd_db",
           lambda i: C.head_relu_bwd_db(dl[i % S], w_head, y[i % S], True))
    record("b_part_outer_product",
           lambda i: dl[i % S].unsqueeze(1) * w_head.unsqueeze(0))

    # (c) fused deep+wide SGD scatter on the strided gradient slice
    record("c_scatter_flat_ids", lambda i: C.emb_bwd_sgd_fused_wide(
        table, wide, flat[i % S], gbuf[i % S][:, PAD:], gw[i % S], LR, 1.0))
    record("c_scatter_raw_ids+offsets", lambda i: C.emb_bwd_sgd_fused_wide(
        table, wide, ids[i % S].reshape(-1), gbuf[i % S][:, PAD:],
        gw[i % S], LR, 1.0, offsets))

    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)),
                    exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
