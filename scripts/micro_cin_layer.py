#!/usr/bin/env python3
"""Micro-benchmark of the CIN-layer kernels at the Criteo shape (m=27, D=16,
bf16): a middle layer (H_in = H_out = 128) and the first layer (H_in = 27,
x is x0's buffer), at --batch examples (65536 unless given: the torch
composition's fp32 intermediates, about 5 x B*H_in*m*D*4 bytes in the
backward, then still fit).

Timed per shape, kernels and the torch composition in the same process:
  (a) _C.cin_layer_fwd            (d) composition forward
  (b) _C.cin_layer_bwd_data       (e) composition data gradients
  (c) _C.cin_layer_bwd_weight     (f) composition weight gradient

Each figure is the median over --repeats windows of --iters calls (device
events around each window, after a warm-up window), with min..max as the
spread.  Calls rotate over --sets independent input sets.  Next to each time
the script prints the bytes the OPERATION must move and the TFLOP/s of its
GEMM (2*B*D*H_out*H_in*m flop), both counted from the shapes, and once per
shape the size of the bf16 outer product the composition materialises.
--json PATH also writes the numbers to a file."""

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


def ref_data(g, x0, x, w, m):
    """(dx, dx0) of the composition."""
    x0f, xf, wf, _ = ops._cin_layer_parts(x0, x, w, m)
    b = x0.shape[0]
    du = torch.einsum("bhc,hij->bijc", g.float().view(b, w.shape[0], -1), wf)
    return ((du * x0f.unsqueeze(1)).sum(2).to(x.dtype),
            (du * xf.unsqueeze(2)).sum(1).to(x0.dtype))


def ref_weight(g, x0, x, w, m):
    z = ops._cin_layer_parts(x0, x, w, m)[3]
    return torch.einsum("bhc,bijc->hij",
                        g.float().view(x0.shape[0], w.shape[0], -1),
                        z).to(w.dtype)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--fields", type=int, default=27)
    ap.add_argument("--dim", type=int, default=16)
    ap.add_argument("--maps", type=int, default=128)
    ap.add_argument("--sets", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    B, m, D, H, S = args.batch, args.fields, args.dim, args.maps, args.sets
    bf16 = torch.bfloat16
    res = {"batch": B, "fields": m, "dim": D, "sets": S, "iters": args.iters,
           "repeats": args.repeats}

    def rand(*shape):
        return torch.randn(*shape, device="cuda").to(bf16)

    for label, h_in in (("middle", H), ("first", m)):
        x0 = [rand(B, m * D) for _ in range(S)]
        x = x0 if h_in == m else [rand(B, h_in * D) for _ in range(S)]
        g = [rand(B, H * D) for _ in range(S)]
        w = rand(H, h_in, m) * (h_in * m) ** -0.5
        assert ops.cin_layer_kernel_ok(x0[0], x[0], w, m)
        el = 2 * B * D
        io = {"fwd": el * (m + h_in + H), "data": el * (H + 2 * m + 2 * h_in),
              "weight": el * (H + m + h_in)}
        flop = 2.0 * B * D * H * h_in * m
        print(f"-- {label}: B={B} m={m} D={D} H_in={h_in} H_out={H}; the "
              f"composition's bf16 outer product is "
              f"{B * h_in * m * D * 2 / 1e9:.2f} GB", flush=True)

        def record(name, fn, nbytes):
            med, lo, hi = timed(fn, args.iters, args.repeats)
            res[f"{label}_{name}"] = {
                "median_us": round(med, 1), "min_us": round(lo, 1),
                "max_us": round(hi, 1), "bytes": int(nbytes),
                "gemm_tflops": round(flop / med / 1e6, 2)}
            print(f"{name:22s} {med:10.1f} us  ({lo:.1f} .. {hi:.1f})  "
                  f"{nbytes / 1e6:7.1f} MB  {flop / med / 1e6:7.2f} TFLOP/s",
                  flush=True)

        C = ops._C
        record("a_kernel_fwd",
               lambda i: C.cin_layer_fwd(x0[i % S], x[i % S], w, 0),
               io["fwd"])
        record("b_kernel_bwd_data",
               lambda i: C.cin_layer_bwd_data(g[i % S], x0[i % S], x[i % S],
                                              w, 0), io["data"])
        record("c_kernel_bwd_weight",
               lambda i: C.cin_layer_bwd_weight(g[i % S], x0[i % S],
                                                x[i % S], w, 0),
               io["weight"])
        record("d_composition_fwd",
               lambda i: ops._cin_layer_ref(x0[i % S], x[i % S], w, m),
               io["fwd"])
        record("e_composition_data",
               lambda i: ref_data(g[i % S], x0[i % S], x[i % S], w, m),
               io["data"])
        record("f_composition_weight",
               lambda i: ref_weight(g[i % S], x0[i % S], x[i % S], w, m),
               io["weight"])
        del x0, x, g
        torch.cuda.empty_cache()

    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)),
                    exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
