#!/usr/bin/env python3
"""Micro-benchmark of the narrow-output weight-gradient kernel
(_C.wgrad_narrow, bf16 output) against the library call it replaces,
dz.t().matmul(x), per (N, M) in --shapes at each batch in --batches.

Per case: the library, the tiled kernel where _custom_wgrad_kernel already
takes the shape, the kernel under its own split plan (splitk = 0), and the
kernel at each slab count in --splitk.  Each figure is the median
over --repeats windows of --iters calls (device events around each window,
after a warm-up window), with min..max as the spread.  Calls rotate over
--sets independent input sets.  Next to each time: the bytes the OPERATION
must move (both operands once, the bf16 result once).  The last column
applies the routing rule: the kernel passes where its median lies below the
library's by more than the larger of the two spreads.  --json PATH also
writes the numbers to a file."""

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scripts.micro_cross_layer import timed  # noqa: E402
from tf_yarn_amd import ops  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+",
                    default=["432x64", "64x432", "432x128", "128x432",
                             "16x256"])
    ap.add_argument("--batches", type=int, nargs="+", default=[65536, 4096])
    ap.add_argument("--splitk", type=int, nargs="*",
                    default=[32, 64, 128, 256])
    ap.add_argument("--sets", type=int, default=6)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    S = args.sets
    res = {"sets": S, "iters": args.iters, "repeats": args.repeats}

    for B in args.batches:
        for shape in args.shapes:
            N, M = (int(v) for v in shape.split("x"))
            dz = [torch.randn(B, N, device="cuda").bfloat16()
                  for _ in range(S)]
            x = [torch.randn(B, M, device="cuda").bfloat16()
                 for _ in range(S)]
            nbytes = 2 * (B * (N + M) + N * M)
            runs = {"lib": lambda i: dz[i % S].t().matmul(x[i % S])}
            # a shape the tiled kernels already take keeps its kernel:
            # timed for the record, the narrow kernel is never asked
            tiled = ops._custom_wgrad_kernel(dz[0], x[0])
            if tiled is not None:
                runs["tiled_" + tiled.__name__] = (
                    lambda i: tiled(dz[i % S], x[i % S], 0, True, None))
            for sk in [0] + args.splitk:
                runs[f"kernel_sk{sk}"] = (
                    lambda i, sk=sk: ops._C.wgrad_narrow(dz[i % S], x[i % S],
                                                         sk, True))
            case = res[f"b{B}_{shape}"] = {}
            for name, fn in runs.items():
                med, lo, hi = timed(fn, args.iters, args.repeats)
                case[name] = {"median_us": round(med, 1),
                              "min_us": round(lo, 1), "max_us": round(hi, 1)}
                print(f"B={B:6d} {shape:8s} {name:13s} {med:8.1f} us  "
                      f"({lo:.1f} .. {hi:.1f})  "
                      f"{nbytes / med / 1e6:6.3f} TB/s", flush=True)
            lib, ker = case["lib"], case["kernel_sk0"]
            spread = max(lib["max_us"] - lib["min_us"],
                         ker["max_us"] - ker["min_us"])
            gain = lib["median_us"] - ker["median_us"]
            case["routed"] = gain > spread
            print(f"B={B:6d} {shape:8s} gain {gain:.1f} us against spread "
                  f"{spread:.1f}: {'PASS' if gain > spread else 'no'}",
                  flush=True)

    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)),
                    exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
