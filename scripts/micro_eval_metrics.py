#!/usr/bin/env python3
"""Micro-benchmark of the streaming eval-state update at one eval batch
(n = 65536 by default), bf16 and fp32 logits:

  * ``ops.binary_eval_update``: the one-pass HIP kernel
    (csrc/eval_metrics.hip);
  * the eager-torch composition that leaves the same state on the GPU:
    sigmoid, BCE-with-logits, the bucket index, one ``bincount`` per class
    (boolean-mask indexing, which waits for the device), tp / fp / loss /
    sigmoid sums, all added into the same three state tensors.  It skips the
    NaN screen the kernel does, which only flatters it.

Before timing, the two are checked against each other on the timed inputs
(histogram and counts equal, sums to 1e-5).  The method is the project's:
each figure is the median over --repeats windows of --iters calls (device
events around each window, after a warm-up window), min..max as the spread,
calls rotate over --sets independent input sets, and the two sides
alternate window by window.  --md PATH writes the table as markdown,
--json PATH the raw numbers."""

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tf_yarn_amd import ops  # noqa: E402


def eager_update(z, y, state):
    z = z.float()
    sig = torch.sigmoid(z)
    loss = torch.nn.functional.binary_cross_entropy_with_logits(
        z, y, reduction="none")
    k = torch.floor((z + 16.0) * 128.0).clamp_(
        0.0, ops.EVAL_BUCKETS - 1.0).to(torch.int64)
    pos = y >= 0.5
    hot = z > 0
    state.hist[0] += torch.bincount(k[~pos], minlength=ops.EVAL_BUCKETS)
    state.hist[1] += torch.bincount(k[pos], minlength=ops.EVAL_BUCKETS)
    state.counts += torch.stack([
        torch.ones_like(k).sum(), torch.zeros_like(k).sum(),
        (pos & hot).sum(), (~pos & hot).sum()])
    state.sums[0, 0] += loss.double().sum()
    state.sums[0, 1] += sig.double().sum()


def window(fn, iters):
    """us per call over one event-timed window of `iters` calls."""
    t0 = torch.cuda.Event(enable_timing=True)
    t1 = torch.cuda.Event(enable_timing=True)
    t0.record()
    for i in range(iters):
        fn(i)
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--sets", type=int, default=6)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--json", default=None)
    ap.add_argument("--md", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    n, S = args.n, args.sets
    res = {"n": n, "sets": S, "iters": args.iters, "repeats": args.repeats,
           "device": torch.cuda.get_device_name(0), "rows": {}}
    rows = []
    for name, dtype in (("bf16", torch.bfloat16), ("fp32", torch.float32)):
        g = torch.Generator().manual_seed(0)
        zs = [(torch.randn(n, generator=g) * 3.0).to(dtype).cuda()
              for _ in range(S)]
        ys = [(torch.rand(n, generator=g) < 0.3).float().cuda()
              for _ in range(S)]
        a, b = ops.BinaryEvalState("cuda"), ops.BinaryEvalState("cuda")
        for z, y in zip(zs, ys):
            ops.binary_eval_update(z, y, a)
            eager_update(z, y, b)
        assert torch.equal(a.hist, b.hist) and torch.equal(a.counts, b.counts)
        torch.testing.assert_close(a.sums.sum(0), b.sums.sum(0), rtol=1e-5,
                                   atol=0)

        sides = {
            "kernel": lambda i: ops.binary_eval_update(zs[i % S], ys[i % S],
                                                       a),
            "eager": lambda i: eager_update(zs[i % S], ys[i % S], b),
        }
        times = {k: [] for k in sides}
        for k, fn in sides.items():  # warm-up window
            window(fn, args.iters)
        for _ in range(args.repeats):
            for k, fn in sides.items():
                times[k].append(window(fn, args.iters))
        row = {}
        for k, t in times.items():
            row[k] = {"median_us": round(statistics.median(t), 1),
                      "min_us": round(min(t), 1), "max_us": round(max(t), 1)}
        row["eager_over_kernel"] = round(
            row["eager"]["median_us"] / row["kernel"]["median_us"], 2)
        res["rows"][name] = row
        rows.append((name, row))
        print(name, json.dumps(row), flush=True)

    lines = [
        "| logits | binary_eval_update (us) | eager torch (us) | eager / "
        "kernel |", "|---|---|---|---|"]
    for name, row in rows:
        kk, ee = row["kernel"], row["eager"]
        lines.append(
            f"| {name} | {kk['median_us']} ({kk['min_us']} .. "
            f"{kk['max_us']}) | {ee['median_us']} ({ee['min_us']} .. "
            f"{ee['max_us']}) | {row['eager_over_kernel']} |")
    table = "\n".join(lines)
    print(table)
    for path, text in ((args.md, table + "\n"),
                       (args.json, json.dumps(res, indent=1))):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as f:
                f.write(text)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
