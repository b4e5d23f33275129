#!/usr/bin/env python3
"""Micro-benchmark of the stateful sparse apply (Adagrad, FTRL, lazy Adam)
at the bench shape (b=65536, 26 features x 1M rows, dim 16 deep + dim 1
wide, bf16 grads).  --rule picks the update rule: adagrad (both tables), ftrl
(both tables), adagrad+ftrl (deep Adagrad, wide FTRL: the wide-and-deep
recipe), rowwise+adagrad / rowwise+ftrl (row-wise Adagrad on the deep
table, one state value per row, with that wide rule) or rowwise (the deep
table alone, no wide companion), lazy_adam (both tables) or lazy_adam_ftrl
(deep lazy Adam, wide FTRL).  A lazy-Adam side is built anew for every
call, with the next step count, as the model builds it.  The three row-wise
settings also time pass 2 of their element-wise counterpart on the same
tables in the same process, before and after a second row-wise window.

Timed, on identical inputs:
  * the fused deep+wide update: pass 1 (atomic accumulate, the existing
    emb_bwd_sgd_fused_wide kernel on the accumulators), pass 2 (claim +
    apply, sparse_adagrad.hip), and both together through the public op;
  * the existing fused deep+wide SGD scatter (context, not a target:
    pass 1 alone is the same atomic traffic);
  * a torch baseline on the GPU: torch.unique (sort) + index_add_ +
    row gather / the same rule elementwise / index_copy_ for both tables.

Each figure is the median over --repeats windows of --iters calls (device
events around each window, after a warm-up window), with min..max as the
spread.  --zipf A draws ids from a Zipf(A) law instead of uniform.
--json PATH also writes the numbers to a file."""

import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tf_yarn_amd import ops  # noqa: E402

F = 26
DIM = 16
LR, EPS = 0.01, 1e-10
L1, L2 = 0.001, 0.001  # FTRL
BETA1, BETA2 = 0.9, 0.999  # lazy Adam
# --rule's names -> the ops' rule names
RULE_NAMES = {"adagrad": "adagrad", "ftrl": "ftrl",
              "rowwise": "rowwise_adagrad", "lazy_adam": "lazy_adam"}
# --rule settings whose name is not "deep+wide"
RULE_SETTINGS = {"lazy_adam": ("lazy_adam", "lazy_adam"),
                 "lazy_adam_ftrl": ("lazy_adam", "ftrl")}


def timed(fn, iters, repeats):
    """us per call: (median, min, max) over `repeats` event-timed windows."""
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        t0 = torch.cuda.Event(enable_timing=True)
        t1 = torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(iters):
            fn()
        t1.record()
        torch.cuda.synchronize()
        out.append(t0.elapsed_time(t1) * 1e3 / iters)
    return statistics.median(out), min(out), max(out)


def make_ids(batch, rows_per, zipf, seed):
    rng = np.random.default_rng(seed)
    if zipf > 0:
        local = (rng.zipf(zipf, size=(batch, F)) - 1) % rows_per
    else:
        local = rng.integers(0, rows_per, size=(batch, F))
    offs = (np.arange(F, dtype=np.int64) * rows_per)[None, :]
    return torch.from_numpy((local + offs).reshape(-1)).cuda()


def _baseline_rows(rule, table, states, uniq, g):
    """One table of the torch baseline: gather the unique rows, apply the
    rule elementwise, copy back.  The FTRL rule is the one `ops` uses."""
    w = table.index_select(0, uniq)
    if rule == "rowwise":
        ss = (g * g).sum(dim=1)
        s = states[0].index_select(0, uniq) + ss / torch.full_like(ss, DIM)
        states[0].index_copy_(0, uniq, s)
        table.index_copy_(0, uniq, w.addcdiv_(
            g, s.sqrt_().add_(EPS).unsqueeze(1), value=-LR))
        return
    if rule == "adagrad":
        s = states[0].index_select(0, uniq).addcmul_(g, g)
        states[0].index_copy_(0, uniq, s)
        table.index_copy_(0, uniq, w.addcdiv_(g, s.sqrt_().add_(EPS),
                                              value=-LR))
        return
    if rule == "lazy_adam":
        # the rule of ops._lazy_adam_rows_ref at a fixed step count
        step_size = LR * (1 - BETA2 ** 10) ** 0.5 / (1 - BETA1 ** 10)
        m = states[0].index_select(0, uniq)
        v = states[1].index_select(0, uniq)
        m = m + (1 - BETA1) * (g - m)
        v = v + (1 - BETA2) * (g * g - v)
        states[0].index_copy_(0, uniq, m)
        states[1].index_copy_(0, uniq, v)
        table.index_copy_(0, uniq, w - (step_size * m) / (v.sqrt() + EPS))
        return
    n, z, w = ops._ftrl_rule(g, states[0].index_select(0, uniq),
                             states[1].index_select(0, uniq), w, LR, L1, L2)
    states[0].index_copy_(0, uniq, n)
    states[1].index_copy_(0, uniq, z)
    table.index_copy_(0, uniq, w)


def torch_baseline(rules, table, states, wide, wide_states, ids, grad, gw):
    uniq, inv = torch.unique(ids, return_inverse=True)
    g = torch.zeros(uniq.numel(), DIM, device=ids.device)
    g.index_add_(0, inv, grad.float())
    _baseline_rows(rules[0], table, states, uniq, g)
    if len(rules) == 1:
        return
    g_div = ids.numel() // gw.numel()
    gwide = torch.zeros(uniq.numel(), device=ids.device)
    gwide.index_add_(0, inv, gw.float().repeat_interleave(g_div))
    _baseline_rows(rules[1], wide.reshape(-1),
                   [s.reshape(-1) for s in wide_states], uniq, gwide)


def make_states(rule, table):
    if rule == "rowwise":
        return [torch.zeros(table.shape[0], device=table.device)]
    if rule == "adagrad":
        return [torch.zeros_like(table)]
    if rule == "lazy_adam":
        return [torch.zeros_like(table), torch.zeros_like(table)]
    return [torch.full_like(table, 0.1), torch.zeros_like(table)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--rows-per-table", type=int, default=1_000_000)
    ap.add_argument("--zipf", type=float, default=0.0,
                    help="Zipf exponent (> 1) for the ids; 0 = uniform")
    ap.add_argument("--rule", default="adagrad",
                    choices=["adagrad", "ftrl", "adagrad+ftrl", "rowwise",
                             "rowwise+adagrad", "rowwise+ftrl", "lazy_adam",
                             "lazy_adam_ftrl"],
                    help="update rule of the deep[+wide] table")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    rules = RULE_SETTINGS.get(args.rule) or tuple(args.rule.split("+"))
    if len(rules) == 1 and args.rule != "rowwise":
        rules *= 2
    pair = len(rules) == 2
    tag = args.rule.replace("+", "_")

    torch.manual_seed(0)
    n_rows = args.rows_per_table * F
    ids = make_ids(args.batch, args.rows_per_table, args.zipf, seed=0)
    n = ids.numel()
    grad = torch.randn(n, DIM, device="cuda").to(torch.bfloat16)
    gw = torch.randn(args.batch, device="cuda").to(torch.bfloat16)
    table = torch.randn(n_rows, DIM, device="cuda")
    wide = torch.randn(n_rows, 1, device="cuda")
    states = make_states(rules[0], table)
    wide_states = make_states(rules[1], wide) if pair else []
    ws = ops.SparseWorkspace(table, wide)
    uniq = int(torch.unique(ids).numel())
    C = ops._C

    res = {"rule": args.rule, "batch": args.batch, "rows": n_rows,
           "updates": n, "unique_rows": uniq, "zipf": args.zipf,
           "iters": args.iters, "repeats": args.repeats}

    def record(name, fn):
        med, lo, hi = timed(fn, args.iters, args.repeats)
        res[name] = {"median_us": round(med, 1), "min_us": round(lo, 1),
                     "max_us": round(hi, 1)}
        print(f"{name:32s} {med:8.1f} us  ({lo:.1f} .. {hi:.1f})",
              flush=True)

    steps = {}  # id(table) -> updates applied, for the lazy-Adam sides

    def adam_tail(rule, tbl):
        """(beta1, beta2, next step count) behind a lazy-Adam side."""
        if rule != "lazy_adam":
            return ()
        steps[id(tbl)] = steps.get(id(tbl), 0) + 1
        return (BETA1, BETA2, steps[id(tbl)])

    def side(rule, tbl, sts, g):
        """One table's side under `rule`, this script's name for it."""
        return ops.SparseSide(RULE_NAMES[rule], tbl, tuple(sts), g, LR, EPS,
                              L1, L2, *adam_tail(rule, tbl))

    def pass2_of(deep_rule, deep_states):
        """Pass 2 alone, straight on the C++ entry: sides without
        gradients, the wide companion whenever --rule has one."""
        def c_side(rule, tbl, sts, acc):
            return (RULE_NAMES[rule], tbl, list(sts), acc, None, LR, EPS,
                    L1, L2) + adam_tail(rule, tbl)

        def sides():
            return (c_side(deep_rule, table, deep_states, ws.acc),
                    c_side(rules[1], wide, wide_states, ws.wide_acc)
                    if pair else None)
        if "lazy_adam" in (deep_rule,) + rules[1:]:
            # the step count differs from call to call
            return lambda: C.emb_bwd_sparse(*sides(), ws.stamp, ids,
                                            ws.next_epoch(), 1.0)
        d, w = sides()
        return lambda: C.emb_bwd_sparse(d, w, ws.stamp, ids,
                                        ws.next_epoch(), 1.0)

    def update(workspace=ws, **sides):
        """The public op; the sides are built per call, as the
        emb_bwd_<rule>* wrappers build them."""
        return lambda: ops.emb_bwd_sparse(
            ids, workspace=workspace,
            **{k: side(*v) for k, v in sides.items()})

    deep_side = (rules[0], table, states, grad)
    wide_side = (rules[1], wide, wide_states, gw) if pair else None
    pass2 = pass2_of(rules[0], states)

    record("sgd_fused_wide", lambda: C.emb_bwd_sgd_fused_wide(
        table, wide, ids, grad, gw, LR, 1.0))
    if pair:
        record(f"{tag}_pass1_accumulate", lambda: C.emb_bwd_sgd_fused_wide(
            ws.acc, ws.wide_acc, ids, grad, gw, -1.0, 1.0))
    else:  # the deep table alone accumulates through emb_bwd_dense
        record(f"{tag}_pass1_accumulate",
               lambda: C.emb_bwd_dense(ws.acc, ids, grad, 1.0))
    # consumes the accumulated sums once, then runs on a clean
    # accumulator: same claims and row traffic every call
    record(f"{tag}_pass2_claim_apply", pass2)
    assert not ws.acc.any() and not ws.wide_acc.any()
    if pair:
        record(f"{tag}_fused_wide_total",
               update(deep=deep_side, wide=wide_side))
        record(f"{tag}_deep_only", update(deep=deep_side))
        record(f"{tag}_wide_only",
               update(workspace=ws.wide_view(), wide=wide_side))
        if rules[0] == "rowwise":
            # the element-wise pair with the same wide rule on the same
            # tables, same process: figures of two processes differ by more
            # than the rules do
            elem = torch.zeros_like(table)
            elem_pass2 = pass2_of("adagrad", [elem])
            record("elementwise_pair_pass2_claim_apply", elem_pass2)
            record(f"{tag}_pass2_claim_apply_again", pass2)
            record("elementwise_pair_pass2_claim_apply_again", elem_pass2)
            del elem
    else:
        record(f"{tag}_total", update(deep=deep_side))
        # element-wise Adagrad on the same deep table, same process
        elem = torch.zeros_like(table)
        record("adagrad_deep_pass2_claim_apply",
               pass2_of("adagrad", [elem]))
        record("adagrad_deep_total",
               update(deep=("adagrad", table, [elem], grad)))
        record(f"{tag}_pass2_claim_apply_again", pass2)
        del elem
    record("torch_unique_index_add", lambda: torch_baseline(
        rules, table, states, wide, wide_states, ids, grad, gw))

    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)),
                    exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
