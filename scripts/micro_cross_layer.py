#!/usr/bin/env python3
"""Micro-benchmark of the cross-layer kernels at the Criteo shape
(b=65536, D = 16 + 26*16 = 432, bf16).

Timed:
  (a)  _C.cross_fwd with v (training);
  (a') _C.cross_fwd without v (inference);
  (b)  _C.cross_bwd_pre (dz, dx0, dbias in one pass);
  (c)  the whole backward: (b), addmm for dx, _linear_wgrad for dW;
  (d)  the best unfused forward without the kernel: _C.lt_linear(x, W, b,
       False) followed by the two torch bf16 elementwise ops;
  (e)  autograd of the fp32 composition (ops._cross_layer_ref).

Each figure is the median over --repeats windows of --iters calls (device
events around each window, after a warm-up window), with min..max as the
spread.  Calls rotate over --sets independent input sets, so inputs come
from HBM and not from a cache the previous call warmed.  Next to each time
the script prints the bytes the OPERATION must move, counted from the
shapes, and the TF of its GEMMs (2*B*D*D each).  --json PATH also writes
the numbers to a file."""

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
    ap.add_argument("--dim", type=int, default=432)
    ap.add_argument("--sets", type=int, default=6)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    B, D, S = args.batch, args.dim, args.sets
    bf16 = torch.bfloat16

    def rand(*shape, scale=1.0):
        return [(torch.randn(*shape, device="cuda") * scale).to(bf16)
                for _ in range(S)]

    x0, x, g = rand(B, D), rand(B, D), rand(B, D)
    w, bias = rand(D, D, scale=D ** -0.5), rand(D)
    assert ops.cross_layer_kernel_ok(x0[0], x[0], w[0], bias[0])
    v = [ops._C.cross_fwd(x0[k], x[k], w[k], bias[k], True)[1]
         for k in range(S)]
    # leaves and retained graphs for (e)
    leaves = [[t[k].clone().requires_grad_() for t in (x0, x, w, bias)]
              for k in range(S)]
    outs = [ops._cross_layer_ref(*leaves[k]) for k in range(S)]

    mat = B * D * 2                 # one [B, D] bf16 operand
    wb = D * D * 2 + D * 2          # weight and bias
    gemm = 2.0 * B * D * D
    res = {"batch": B, "dim": D, "sets": S, "iters": args.iters,
           "repeats": args.repeats}

    def record(name, fn, nbytes, flop):
        med, lo, hi = timed(fn, args.iters, args.repeats)
        res[name] = {"median_us": round(med, 1), "min_us": round(lo, 1),
                     "max_us": round(hi, 1), "bytes": int(nbytes),
                     "tb_per_s": round(nbytes / med / 1e6, 3),
                     "tflops": round(flop / med / 1e6, 1)}
        print(f"{name:28s} {med:9.1f} us  ({lo:.1f} .. {hi:.1f})  "
              f"{nbytes / 1e6:7.1f} MB  {nbytes / med / 1e6:6.3f} TB/s  "
              f"{flop / med / 1e6:6.1f} TF", flush=True)

    def backward(i):
        k = i % S
        dz, dx0, dbias = ops._C.cross_bwd_pre(g[k], x0[k], v[k])
        dx = torch.addmm(g[k], dz, w[k])
        return dx0, dx, ops._linear_wgrad(dz, x[k], w[k]), dbias

    def unfused(i):
        k = i % S
        return x0[k] * ops._C.lt_linear(x[k], w[k], bias[k], False) + x[k]

    record("a_cross_fwd_v",
           lambda i: ops._C.cross_fwd(x0[i % S], x[i % S], w[i % S],
                                      bias[i % S], True),
           4 * mat + wb, gemm)
    record("a2_cross_fwd_no_v",
           lambda i: ops._C.cross_fwd(x0[i % S], x[i % S], w[i % S],
                                      bias[i % S], False),
           3 * mat + wb, gemm)
    record("b_cross_bwd_pre",
           lambda i: ops._C.cross_bwd_pre(g[i % S], x0[i % S], v[i % S]),
           5 * mat + D * 2, 0.0)
    # g, x0, v, x in; dx0, dx, dW, dbias out (dz stays an intermediate)
    record("c_backward", backward, 6 * mat + 2 * wb, 2 * gemm)
    record("d_lt_linear_mul_add", unfused, 3 * mat + wb, gemm)
    record("e_fp32_composition_bwd",
           lambda i: torch.autograd.grad(outs[i % S], leaves[i % S],
                                         g[i % S], retain_graph=True),
           6 * mat + 2 * wb, 2 * gemm)

    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)),
                    exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
