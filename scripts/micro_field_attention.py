#!/usr/bin/env python3
"""Micro-benchmark of the field-attention kernels at the Criteo shape
(B=65536, N=27, H=2, d=16, bf16).

Timed:
  (a) _C.field_attention_fwd;
  (b) _C.field_attention_bwd (dqkv from qkv and grad_out);
  (c) the torch composition forward (ops._field_attention_ref);
  (d) the torch composition backward (ops._field_attention_ref_bwd).

Each figure is the median over --repeats windows of --iters calls (device
events around each window, after a warm-up window), with min..max as the
spread.  Calls rotate over --sets independent input sets, so inputs come
from HBM and not from a cache the previous call warmed.  Next to each time
the script prints the bytes the OPERATION must move, counted from the
shapes.  --json PATH also writes the numbers to a file."""

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tf_yarn_amd import ops  # noqa: E402


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
    ap.add_argument("--fields", type=int, default=27)
    ap.add_argument("--heads", type=int, default=2)
    ap.add_argument("--head-dim", type=int, default=16)
    ap.add_argument("--sets", type=int, default=6)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    B, N, H, d, S = (args.batch, args.fields, args.heads, args.head_dim,
                     args.sets)
    rows, hd, scale = B * N, H * d, d ** -0.5
    qkv = [torch.randn(rows, 3 * hd, device="cuda").to(torch.bfloat16)
           for _ in range(S)]
    g = [torch.randn(rows, hd, device="cuda").to(torch.bfloat16)
         for _ in range(S)]
    assert ops.field_attention_kernel_ok(qkv[0], N, H)

    tok = rows * hd * 2             # one [B*N, H*d] bf16 operand
    res = {"batch": B, "fields": N, "heads": H, "head_dim": d, "sets": S,
           "iters": args.iters, "repeats": args.repeats}

    def record(name, fn, nbytes):
        med, lo, hi = timed(fn, args.iters, args.repeats)
        res[name] = {"median_us": round(med, 1), "min_us": round(lo, 1),
                     "max_us": round(hi, 1), "bytes": int(nbytes),
                     "tb_per_s": round(nbytes / med / 1e6, 3)}
        print(f"{name:24s} {med:9.1f} us  ({lo:.1f} .. {hi:.1f})  "
              f"{nbytes / 1e6:7.1f} MB  {nbytes / med / 1e6:6.3f} TB/s",
              flush=True)

    record("a_kernel_fwd",
           lambda i: ops._C.field_attention_fwd(qkv[i % S], N, H, scale, 0),
           4 * tok)
    record("b_kernel_bwd",
           lambda i: ops._C.field_attention_bwd(g[i % S], qkv[i % S], N, H,
                                                scale, 0),
           7 * tok)
    record("c_composition_fwd",
           lambda i: ops._field_attention_ref(qkv[i % S], N, H, scale),
           4 * tok)
    record("d_composition_bwd",
           lambda i: ops._field_attention_ref_bwd(g[i % S], qkv[i % S], N, H,
                                                  scale),
           7 * tok)

    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)),
                    exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
