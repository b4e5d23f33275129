#!/usr/bin/env python3
"""Micro-benchmark of the backward's column-partial tail at the bench shape
(b=65536, MLP 1024-512-256, 13 dense features padded to 16, bf16):

  (a) the five partial slabs of a step, summed the old way (torch's
      sum(0) + the bf16 cast, MIYARN_TALL_REDUCE=0) against
      reduce_splitk's tall kernel, with 1 and with 4 quad lanes per block;
  (b) the top of the MLP backward: head_relu_bwd_db + col_reduce_dot +
      dl.sum() and their casts, against col_reduce_dot_sum +
      head_relu_bwd_db, against the one-pass head_relu_bwd_grads;
  (c) col_reduce_dot at 65536x16 (the wide-dense head) on the old grid of
      32 blocks with torch's sum against one block per CU with the tall
      kernel, and col_reduce_dot_sum there.

The method is the project's: each figure is the median over --repeats
windows of --iters calls (device events around each window, after a
warm-up window) with min..max as the spread, and calls rotate over --sets
independent input sets.  --json PATH also writes the numbers to a file."""

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tf_yarn_amd import ops  # noqa: E402

WIDTH = 256
# (partial rows, columns, what writes it)
SLABS = [
    (2048, 1024, "dbias mlp.0"),
    (8192, 512, "dbias mlp.1"),
    (8192, 256, "dbias mlp.2"),
    (2048, 256, "col_reduce_dot head"),
    (2048, 16, "col_reduce_dot wide_dense"),
]


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
    res = {"batch": B, "sets": S, "iters": args.iters,
           "repeats": args.repeats}

    def record(name, fn, tall="1"):
        os.environ["MIYARN_TALL_REDUCE"] = tall
        med, lo, hi = timed(fn, args.iters, args.repeats)
        os.environ.pop("MIYARN_TALL_REDUCE")
        res[name] = {"median_us": round(med, 1), "min_us": round(lo, 1),
                     "max_us": round(hi, 1)}
        print(f"{name:52s} {med:8.1f} us  ({lo:.1f} .. {hi:.1f})",
              flush=True)

    # (a) the slabs
    for rows, cols, what in SLABS:
        part = [torch.randn(rows, cols, device="cuda") for _ in range(S)]
        tag = f"a_{rows}x{cols}"
        record(f"{tag}_torch_sum+cast ({what})",
               lambda i: C.reduce_splitk(part[i % S], True), tall="0")
        record(f"{tag}_tall_1_quad_lane",
               lambda i: C.reduce_tall(part[i % S], True, 1))
        record(f"{tag}_tall_4_quad_lanes",
               lambda i: C.reduce_tall(part[i % S], True, 4))
        del part

    # (b) top of the MLP backward
    y = [torch.relu(torch.randn(B, WIDTH, device="cuda")).to(bf16)
         for _ in range(S)]
    dl = [torch.randn(B, device="cuda").to(bf16) for _ in range(S)]
    w_head = (torch.randn(WIDTH, device="cuda") * 0.06).to(bf16)

    def head_separate(i):
        k = i % S
        C.col_reduce_dot(y[k], dl[k]).to(bf16)
        dl[k].sum().reshape(1).to(bf16)
        C.head_relu_bwd_db(dl[k], w_head, y[k], True)

    def head_dot_sum(i):
        k = i % S
        C.col_reduce_dot_sum(y[k], dl[k], True)
        C.head_relu_bwd_db(dl[k], w_head, y[k], True)

    record("b_head_db+col_reduce_dot+sum+casts, torch sums", head_separate,
           tall="0")
    record("b_head_db+col_reduce_dot+sum+casts", head_separate)
    record("b_head_db+col_reduce_dot_sum", head_dot_sum)
    record("b_head_relu_bwd_grads",
           lambda i: C.head_relu_bwd_grads(dl[i % S], w_head, y[i % S], True))
    record("b_part_head_relu_bwd_db",
           lambda i: C.head_relu_bwd_db(dl[i % S], w_head, y[i % S], True))
    record("b_part_col_reduce_dot_sum",
           lambda i: C.col_reduce_dot_sum(y[i % S], dl[i % S], True))
    del y

    # (c) the wide-dense head
    x = [torch.randn(B, 16, device="cuda").to(bf16) for _ in range(S)]
    record("c_col_reduce_dot_65536x16_32_blocks+torch_sum",
           lambda i: C.col_reduce_dot(x[i % S], dl[i % S]), tall="0")
    record("c_col_reduce_dot_65536x16_256_blocks+tall",
           lambda i: C.col_reduce_dot(x[i % S], dl[i % S]))
    record("c_col_reduce_dot_sum_65536x16",
           lambda i: C.col_reduce_dot_sum(x[i % S], dl[i % S], True))

    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)),
                    exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
