#!/usr/bin/env python3
"""Micro-benchmark of the dot-interaction kernels at the flagship shape
(b=65536, N = 26 + 1 vectors of dim 16, bf16, W = 368 output columns).

Timed:
  (a) _C.dot_interaction_fwd;
  (b) _C.dot_interaction_bwd (both gradients, one kernel);
  (c) the torch composition forward (cat, bmm in bf16, the triangle gather
      through cached indices, cat with the pad);
  (d) the composition's backward through autograd (grad of (c)).

Each figure is the median over --repeats windows of --iters calls (device
events around each window, after a warm-up window), with min..max as the
spread.  Calls rotate over --sets independent input sets, so inputs come
from HBM and not from a cache the previous call warmed.  Next to each time
the script prints the bytes the OPERATION must move, counted from the
shapes (864 B of operands and 736 B of result per example forward; those
plus the two gradients backward), and the resulting TB/s; the composition
is charged the same count, so its TB/s is a rate of useful bytes, not of
its own intermediates.  --json PATH also writes the numbers to a file."""

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


def composition(dv, emb, idx):
    """The bf16 composition a user would write; `idx` = cached tril pair."""
    b, d = dv.shape
    t = torch.cat([dv, emb], dim=1).reshape(b, -1, d)
    pairs = torch.bmm(t, t.transpose(1, 2))[:, idx[0], idx[1]]
    w = ops.dot_interaction_width(t.shape[1] - 1, d)
    return torch.cat([dv, pairs, pairs.new_zeros(b, w - d - pairs.shape[1])],
                     dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--features", type=int, default=26)
    ap.add_argument("--dim", type=int, default=16)
    ap.add_argument("--sets", type=int, default=6)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    B, F, D, S = args.batch, args.features, args.dim, args.sets
    W = ops.dot_interaction_width(F, D)
    bf16 = torch.bfloat16

    def rand(cols):
        return [torch.randn(B, cols, device="cuda").to(bf16)
                for _ in range(S)]

    dv, emb, g = rand(D), rand(F * D), rand(W)
    assert ops.dot_interaction_kernel_ok(dv[0], emb[0])
    idx = torch.tril_indices(F + 1, F + 1, offset=-1, device="cuda")
    # leaves and retained graphs for (d)
    dv_l = [t.clone().requires_grad_() for t in dv]
    emb_l = [t.clone().requires_grad_() for t in emb]
    outs = [composition(dv_l[k], emb_l[k], idx) for k in range(S)]

    in_b = B * (D + F * D) * 2
    fwd_b = in_b + B * W * 2
    bwd_b = in_b + B * W * 2 + in_b
    res = {"batch": B, "features": F, "dim": D, "width": W, "sets": S,
           "iters": args.iters, "repeats": args.repeats}

    def record(name, fn, nbytes):
        med, lo, hi = timed(fn, args.iters, args.repeats)
        res[name] = {"median_us": round(med, 1), "min_us": round(lo, 1),
                     "max_us": round(hi, 1), "bytes": int(nbytes),
                     "tb_per_s": round(nbytes / med / 1e6, 3)}
        print(f"{name:28s} {med:9.1f} us  ({lo:.1f} .. {hi:.1f})  "
              f"{nbytes / 1e6:7.1f} MB  {nbytes / med / 1e6:6.3f} TB/s",
              flush=True)

    record("a_dot_interaction_fwd",
           lambda i: ops._C.dot_interaction_fwd(dv[i % S], emb[i % S]), fwd_b)
    record("b_dot_interaction_bwd",
           lambda i: ops._C.dot_interaction_bwd(g[i % S], dv[i % S],
                                                emb[i % S]), bwd_b)
    record("c_torch_composition_fwd",
           lambda i: composition(dv[i % S], emb[i % S], idx), fwd_b)
    record("d_torch_composition_bwd",
           lambda i: torch.autograd.grad(
               outs[i % S], (dv_l[i % S], emb_l[i % S]), g[i % S],
               retain_graph=True), bwd_b)

    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)),
                    exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
