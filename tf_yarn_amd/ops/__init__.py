"""MI355X HIP kernel library: Python wrappers + CPU references.

Policy (required for the GPU-native check): on a machine with a GPU the
HIP extension MUST be present — ops raise immediately if it failed to
import, instead of silently falling back to eager torch.  On CPU-only
machines (the CI container) the same functions run reference torch
implementations so every numerics test has a CPU baseline.
"""

from __future__ import annotations

import functools
import logging
import math
import os
from typing import NamedTuple, Optional, Tuple

import torch

logger = logging.getLogger(__name__)

try:
    from tf_yarn_amd.ops import _C  # built by setup.py build_ext --inplace
    HAVE_EXT = True
except ImportError as _e:  # pragma: no cover - exercised only sans build
    _C = None
    HAVE_EXT = False
    _IMPORT_ERROR = _e


def _require_ext() -> None:
    if not HAVE_EXT:
        raise RuntimeError(
            "tf_yarn_amd.ops._C is not built but a GPU tensor was passed. "
            "Run `python setup.py build_ext --inplace` "
            f"(import error: {_IMPORT_ERROR})")


def _on_gpu(*tensors: torch.Tensor) -> bool:
    return any(t.is_cuda for t in tensors if isinstance(t, torch.Tensor))


# ---- fused optimizers ------------------------------------------------------

def fused_sgd(param: torch.Tensor, grad: torch.Tensor,
              momentum_buf: Optional[torch.Tensor] = None,
              param_bf16: Optional[torch.Tensor] = None,
              *, lr: float, momentum: float = 0.0, dampening: float = 0.0,
              weight_decay: float = 0.0, nesterov: bool = False,
              first_step: bool = False, grad_scale: float = 1.0) -> None:
    if _on_gpu(param, grad):
        _require_ext()
        _C.fused_sgd(param, grad, momentum_buf, param_bf16, lr, momentum,
                     dampening, weight_decay, nesterov, first_step,
                     grad_scale)
        return
    g = grad.float() * grad_scale
    g = g.add(param, alpha=weight_decay)
    if momentum_buf is not None:
        if first_step:
            momentum_buf.copy_(g)
        else:
            momentum_buf.mul_(momentum).add_(g, alpha=1.0 - dampening)
        g = g.add(momentum_buf, alpha=momentum) if nesterov \
            else momentum_buf.clone()
    param.add_(g, alpha=-lr)
    if param_bf16 is not None:
        param_bf16.copy_(param.to(torch.bfloat16))


def fused_sgd_mt(params, grads, momentum_bufs=None, params_bf16=None,
                 *, lr: float, momentum: float = 0.0,
                 dampening: float = 0.0, weight_decay: float = 0.0,
                 nesterov: bool = False, first_step: bool = False,
                 grad_scale: float = 1.0) -> None:
    """Multi-tensor SGD: one kernel launch per <=24 tensors."""
    if params and params[0].is_cuda:
        _require_ext()
        _C.fused_sgd_mt(list(params), list(grads),
                        list(momentum_bufs) if momentum_bufs else [],
                        list(params_bf16) if params_bf16 else [],
                        lr, momentum, dampening, weight_decay, nesterov,
                        first_step, grad_scale)
        return
    for i, (p, g) in enumerate(zip(params, grads)):
        fused_sgd(p, g,
                  momentum_bufs[i] if momentum_bufs else None,
                  params_bf16[i] if params_bf16 else None,
                  lr=lr, momentum=momentum, dampening=dampening,
                  weight_decay=weight_decay, nesterov=nesterov,
                  first_step=first_step, grad_scale=grad_scale)


def fused_adam(param: torch.Tensor, grad: torch.Tensor,
               exp_avg: torch.Tensor, exp_avg_sq: torch.Tensor,
               param_bf16: Optional[torch.Tensor] = None,
               *, lr: float, beta1: float = 0.9, beta2: float = 0.999,
               eps: float = 1e-8, weight_decay: float = 0.0,
               adamw: bool = False, step: int = 1,
               grad_scale: float = 1.0) -> None:
    if _on_gpu(param, grad):
        _require_ext()
        _C.fused_adam(param, grad, exp_avg, exp_avg_sq, param_bf16, lr,
                      beta1, beta2, eps, weight_decay, adamw, step,
                      grad_scale)
        return
    g = grad.float() * grad_scale
    if adamw:
        param.mul_(1.0 - lr * weight_decay)
    else:
        g = g.add(param, alpha=weight_decay)
    exp_avg.mul_(beta1).add_(g, alpha=1 - beta1)
    exp_avg_sq.mul_(beta2).addcmul_(g, g, value=1 - beta2)
    bc1 = 1 - beta1 ** step
    bc2 = 1 - beta2 ** step
    denom = (exp_avg_sq / bc2).sqrt_().add_(eps)
    param.addcdiv_(exp_avg / bc1, denom, value=-lr)
    if param_bf16 is not None:
        param_bf16.copy_(param.to(torch.bfloat16))


def fused_adagrad(param: torch.Tensor, grad: torch.Tensor,
                  state_sum: torch.Tensor, *, lr: float, eps: float = 1e-10,
                  weight_decay: float = 0.0,
                  grad_scale: float = 1.0) -> None:
    if _on_gpu(param, grad):
        _require_ext()
        _C.fused_adagrad(param, grad, state_sum, lr, eps, weight_decay,
                         grad_scale)
        return
    g = grad.float() * grad_scale
    g = g.add(param, alpha=weight_decay)
    state_sum.addcmul_(g, g, value=1.0)
    param.addcdiv_(g, state_sum.sqrt().add_(eps), value=-lr)


def _check_ftrl_args(lr: float, l1: float, l2: float) -> None:
    if not lr > 0:
        raise ValueError(f"FTRL needs lr > 0, got {lr!r}")
    if not (l1 >= 0 and l2 >= 0):
        raise ValueError(
            f"FTRL needs l1 >= 0 and l2 >= 0, got l1={l1!r}, l2={l2!r}")


def _ftrl_rule(g: torch.Tensor, n: torch.Tensor, z: torch.Tensor,
               w: torch.Tensor, lr: float, l1: float, l2: float):
    """FTRL-proximal (TF ``Ftrl``, ``learning_rate_power=-0.5``, no beta,
    no L2 shrinkage) on same-shaped tensors; returns ``(n', z', w')``.
    ``w'`` is exactly 0 where ``|z'| <= l1`` (which also covers q == 0:
    that needs n' == 0 and l2 == 0, where z' == z == 0)."""
    n_new = n + g * g
    r_new = n_new.sqrt()
    z_new = z + g - (r_new - n.sqrt()) / lr * w
    q = r_new / lr + 2.0 * l2
    w_new = torch.where(z_new.abs() > l1,
                        (torch.sign(z_new) * l1 - z_new) / q,
                        torch.zeros_like(z_new))
    return n_new, z_new, w_new


def fused_ftrl(param: torch.Tensor, grad: torch.Tensor,
               accum: torch.Tensor, linear: torch.Tensor, *, lr: float,
               l1: float = 0.0, l2: float = 0.0,
               grad_scale: float = 1.0) -> None:
    """Dense FTRL-proximal step: EVERY element is recomputed from
    ``(linear, accum)`` every step (TF's dense semantics; the sparse
    tables use :func:`emb_bwd_ftrl`, which only touches the batch's
    rows)."""
    _check_ftrl_args(lr, l1, l2)
    if _on_gpu(param, grad):
        _require_ext()
        _C.fused_ftrl(param, grad, accum, linear, lr, l1, l2, grad_scale)
        return
    g = grad.float() * grad_scale
    n, z, w = _ftrl_rule(g, accum, linear, param, lr, l1, l2)
    accum.copy_(n)
    linear.copy_(z)
    param.copy_(w)


def fused_adadelta(param: torch.Tensor, grad: torch.Tensor,
                   square_avg: torch.Tensor, acc_delta: torch.Tensor,
                   *, lr: float = 1.0, rho: float = 0.9, eps: float = 1e-6,
                   weight_decay: float = 0.0,
                   grad_scale: float = 1.0) -> None:
    if _on_gpu(param, grad):
        _require_ext()
        _C.fused_adadelta(param, grad, square_avg, acc_delta, lr, rho, eps,
                          weight_decay, grad_scale)
        return
    g = grad.float() * grad_scale
    g = g.add(param, alpha=weight_decay)
    square_avg.mul_(rho).addcmul_(g, g, value=1 - rho)
    dx = (acc_delta + eps).sqrt_().div_((square_avg + eps).sqrt()).mul_(g)
    acc_delta.mul_(rho).addcmul_(dx, dx, value=1 - rho)
    param.add_(dx, alpha=-lr)


# ---- embedding -------------------------------------------------------------

def emb_fwd(table: torch.Tensor, ids: torch.Tensor,
            out_bf16: bool = False) -> torch.Tensor:
    """Row gather: out[i, :] = table[ids[i], :] (ids pre-offset, flat)."""
    if _on_gpu(table, ids):
        _require_ext()
        return _C.emb_fwd(table, ids, out_bf16)
    out = table.index_select(0, ids.reshape(-1))
    return out.to(torch.bfloat16) if out_bf16 else out


def emb_bwd_sgd(table: torch.Tensor, ids: torch.Tensor, grad: torch.Tensor,
                *, lr: float, scale: float = 1.0) -> None:
    """table[ids[i], :] -= lr * scale * grad[i, :] (fused sparse update).

    The atomic scatter is the default: the atomic-free sorted kernel
    (`_C.emb_bwd_sgd_sorted`) is 4.6x faster per-kernel, but paying
    torch.sort + a 54 MB gather every step measured NET-slower at the
    bench shape (bench 2.30 vs 1.86 ms/step) — use it only when ids
    arrive pre-sorted."""
    if _on_gpu(table, ids, grad):
        _require_ext()
        _C.emb_bwd_sgd(table, ids.reshape(-1).contiguous(),
                       grad.contiguous(), lr, scale)
        return
    table.index_add_(0, ids.reshape(-1),
                     grad.reshape(ids.numel(), -1).float(),
                     alpha=-lr * scale)


def pick_region_bits(n_rows: int, n_updates: int) -> int:
    """Region size heuristic for the binned scatter: aim for an expected
    per-bin update count around half the LDS hash capacity (1024 for deep
    tables) so dedup almost never overflows into the atomic fallback,
    while keeping enough bins (>2048) to fill all 256 CUs."""
    import math
    if n_updates <= 0:
        return 11
    target = max(1.0, 512.0 * n_rows / n_updates)
    bits = int(math.log2(target))
    return max(7, min(14, bits))


def binned_permutation(ids: torch.Tensor, n_rows: int,
                       region_bits: int):
    """Pass A of the binned scatter (GPU): permutation of update indices
    grouped by 2^region_bits-row table regions + bin start offsets.
    Algorithm spec: tests/test_binned_scatter_spec.py."""
    _require_ext()
    return _C.binned_permutation(ids.reshape(-1).contiguous(), n_rows,
                                 region_bits)


def emb_bwd_sgd_binned(table: torch.Tensor, ids: torch.Tensor,
                       grad: torch.Tensor, *, lr: float,
                       scale: float = 1.0,
                       perm=None, region_bits: int = None) -> None:
    """Binned replacement for :func:`emb_bwd_sgd` (dim-16 tables): LDS
    hash dedup per region + exclusive-owner writeback, no global atomics
    on the hot path.  ``perm`` = (order, starts) from
    :func:`binned_permutation` can be shared between the deep and wide
    tables (same flat ids).  CPU reference: plain index_add_."""
    if not _on_gpu(table, ids, grad):
        table.index_add_(0, ids.reshape(-1),
                         grad.reshape(ids.numel(), -1).float(),
                         alpha=-lr * scale)
        return
    _require_ext()
    ids = ids.reshape(-1).contiguous()
    if perm is None:
        if region_bits is None:
            region_bits = pick_region_bits(table.shape[0], ids.numel())
        perm = _C.binned_permutation(ids, table.shape[0], region_bits)
    order, starts = perm
    _C.emb_bwd_sgd_binned(table, ids, grad.contiguous(), lr, scale,
                          order, starts)


def emb_scatter_sum_binned(table: torch.Tensor, ids: torch.Tensor,
                           grad: torch.Tensor, alpha: float,
                           perm=None, region_bits: int = None) -> None:
    """Binned replacement for :func:`emb_scatter_sum` (scalar wide
    tables): grad for flat update j is ``grad[j // F]``."""
    n = ids.numel()
    g_div = n // grad.numel() if grad.numel() else 1  # empty update
    if not _on_gpu(table, ids, grad):
        expanded = grad.float().reshape(-1, 1).expand(-1, g_div) \
            .reshape(-1)
        table.reshape(-1).index_add_(0, ids.reshape(-1), expanded,
                                     alpha=alpha)
        return
    _require_ext()
    ids = ids.reshape(-1).contiguous()
    if perm is None:
        if region_bits is None:
            region_bits = pick_region_bits(table.shape[0], n)
        perm = _C.binned_permutation(ids, table.shape[0], region_bits)
    order, starts = perm
    _C.emb_scatter_sum_binned(table, ids, grad.contiguous(), g_div,
                              alpha, order, starts)


def emb_bwd_sgd_fused_wide(table: torch.Tensor, wide_table: torch.Tensor,
                           ids: torch.Tensor, grad: torch.Tensor,
                           gw: torch.Tensor, *, lr: float,
                           scale: float = 1.0,
                           offsets: Optional[torch.Tensor] = None) -> None:
    """Fused sparse update of BOTH CTR tables from one pass over the
    shared flat ids:  ``table[ids[i]] -= lr*scale*grad[i]`` and
    ``wide_table[ids[i]] -= lr*scale*gw[i // (n//gw.numel())]``.

    ``grad`` is ``[n, dim]``, or a ``[gw.numel(), (n//gw.numel()) * dim]``
    column slice of a wider row-major buffer (unit column stride): the
    kernel reads such a view in place, with no gather copy first.

    With ``offsets`` (``[F]`` int64), ``ids`` is the raw ``[gw.numel(), F]``
    array of per-feature ids and update ``(b, f)`` goes to row
    ``ids[b, f] + offsets[f]``: the kernel adds the offset itself, so the
    caller needs no pre-added copy of the ids."""
    if _on_gpu(table, ids, grad) and grad.dtype == gw.dtype:
        _require_ext()
        if not (grad.dim() == 2 and grad.stride(1) == 1
                and grad.shape[0] == gw.numel()
                and grad.stride(0) >= grad.shape[1]):
            grad = grad.contiguous()
        _C.emb_bwd_sgd_fused_wide(table, wide_table,
                                  ids.reshape(-1).contiguous(),
                                  grad, gw.contiguous(), lr, scale,
                                  offsets)
        return
    if offsets is not None:
        ids = ids.reshape(gw.numel(), -1) + offsets.unsqueeze(0)
    n = ids.numel()
    g_div = n // gw.numel()
    table.index_add_(0, ids.reshape(-1),
                     grad.reshape(n, -1).float(), alpha=-lr * scale)
    expanded = gw.float().reshape(-1, 1).expand(-1, g_div).reshape(-1)
    wide_table.reshape(-1).index_add_(0, ids.reshape(-1), expanded,
                                      alpha=-lr * scale)


def emb_bwd_dense(grad_table: torch.Tensor, ids: torch.Tensor,
                  grad: torch.Tensor, scale: float = 1.0) -> None:
    if _on_gpu(grad_table, ids, grad):
        _require_ext()
        _C.emb_bwd_dense(grad_table, ids, grad.contiguous(), scale)
        return
    grad_table.index_add_(0, ids.reshape(-1),
                          grad.reshape(ids.numel(), -1).float(),
                          alpha=scale)


# ---- stateful sparse updates (Adagrad, FTRL, lazy Adam, row-wise Adagrad) --

class SparseWorkspace:
    """Device scratch of the accumulate-then-claim sparse kernels for one
    table (optionally with its ``[rows, 1]`` wide companion).  It holds no
    rule state, so one instance, and so one stamp, serves a deep table and
    its wide companion whatever their rules.

    ``acc`` (and ``wide_acc``): fp32, shaped like the table, ALL-ZERO
    between calls — pass 1 scatter-adds into it and pass 2 zeroes every
    row it consumes.  ``stamp``: int32 per row, zero-initialised; a row is
    claimed by exchanging the current ``epoch`` into it.  ``epoch`` starts
    at 1 and advances on every apply launch, so the stamp is never
    cleared (except once per 2^31 launches, when the counter wraps).
    Cost: one extra table-sized fp32 buffer + 4 B/row."""

    _EPOCH_MAX = 2 ** 31 - 2

    def __init__(self, table: torch.Tensor,
                 wide_table: Optional[torch.Tensor] = None):
        self.acc = torch.zeros_like(table)
        self.wide_acc = (torch.zeros_like(wide_table)
                         if wide_table is not None else None)
        self.stamp = torch.zeros(table.shape[0], dtype=torch.int32,
                                 device=table.device)
        self.epoch = 0  # last epoch handed out

    def next_epoch(self) -> int:
        if self.epoch >= self._EPOCH_MAX:
            self.stamp.zero_()
            self.epoch = 0
        self.epoch += 1
        return self.epoch

    def wide_view(self) -> "_WideWorkspaceView":
        """The wide table's single-table face of a deep+wide workspace:
        ``wide_acc`` with the shared stamp and epoch counter."""
        return _WideWorkspaceView(self)


SparseAdagradWorkspace = SparseWorkspace  # the name from before FTRL


class _WideWorkspaceView:
    def __init__(self, ws: SparseWorkspace):
        self._ws = ws

    @property
    def acc(self) -> torch.Tensor:
        return self._ws.wide_acc

    @property
    def stamp(self) -> torch.Tensor:
        return self._ws.stamp

    def next_epoch(self) -> int:
        return self._ws.next_epoch()


def _adagrad_rows_ref(table: torch.Tensor, state_sum: torch.Tensor,
                      flat_ids: torch.Tensor, rows: torch.Tensor,
                      lr: float, eps: float, scale: float) -> None:
    """Reference: coalesce duplicate ids, then one Adagrad step on the
    unique rows (== torch.optim.Adagrad on a coalesced sparse grad)."""
    uniq, inv = torch.unique(flat_ids, return_inverse=True)
    g = torch.zeros(uniq.numel(), rows.shape[1], dtype=torch.float32,
                    device=rows.device)
    g.index_add_(0, inv, rows.float())
    g.mul_(scale)
    s = state_sum.index_select(0, uniq).addcmul_(g, g, value=1.0)
    state_sum.index_copy_(0, uniq, s)
    w = table.index_select(0, uniq).addcdiv_(g, s.sqrt().add_(eps),
                                             value=-lr)
    table.index_copy_(0, uniq, w)


def _ftrl_rows_ref(table: torch.Tensor, accum: torch.Tensor,
                   linear: torch.Tensor, flat_ids: torch.Tensor,
                   rows: torch.Tensor, lr: float, l1: float, l2: float,
                   scale: float) -> None:
    """Reference: coalesce duplicate ids, then one FTRL step on the unique
    rows ONLY (lazy semantics: a dense step would recompute every weight
    from (z, n) and wipe the initial weights of untouched rows)."""
    uniq, inv = torch.unique(flat_ids, return_inverse=True)
    g = torch.zeros(uniq.numel(), rows.shape[1], dtype=torch.float32,
                    device=rows.device)
    g.index_add_(0, inv, rows.float())
    g.mul_(scale)
    n, z, w = _ftrl_rule(g, accum.index_select(0, uniq),
                         linear.index_select(0, uniq),
                         table.index_select(0, uniq), lr, l1, l2)
    accum.index_copy_(0, uniq, n)
    linear.index_copy_(0, uniq, z)
    table.index_copy_(0, uniq, w)


def _rowwise_adagrad_rows_ref(table: torch.Tensor, state_row: torch.Tensor,
                              flat_ids: torch.Tensor, rows: torch.Tensor,
                              lr: float, eps: float, scale: float) -> None:
    """Reference: coalesce duplicate ids, then one row-wise Adagrad step
    on the unique rows.  The mean of squares is a true division by ``dim``
    (tensor / tensor, never a multiply by a reciprocal)."""
    uniq, inv = torch.unique(flat_ids, return_inverse=True)
    dim = rows.shape[1]
    g = torch.zeros(uniq.numel(), dim, dtype=torch.float32,
                    device=rows.device)
    g.index_add_(0, inv, rows.float())
    g.mul_(scale)
    ss = (g * g).sum(dim=1)
    s = state_row.index_select(0, uniq) + ss / torch.full_like(ss, dim)
    state_row.index_copy_(0, uniq, s)
    w = table.index_select(0, uniq).addcdiv_(
        g, s.sqrt().add_(eps).unsqueeze(1), value=-lr)
    table.index_copy_(0, uniq, w)


def _check_lazy_adam_args(lr: float, eps: float, beta1: float, beta2: float,
                          step: int) -> None:
    if not lr > 0:
        raise ValueError(f"lazy Adam needs lr > 0, got {lr!r}")
    if not (0 <= beta1 < 1 and 0 <= beta2 < 1):
        raise ValueError("lazy Adam needs 0 <= beta < 1 for both betas, got "
                         f"beta1={beta1!r}, beta2={beta2!r}")
    if not eps >= 0:
        raise ValueError(f"lazy Adam needs eps >= 0, got {eps!r}")
    if not (isinstance(step, int) and step >= 1):
        raise ValueError(
            "lazy Adam needs an int step >= 1 (the count of updates applied "
            f"to the table, this one included), got {step!r}")


def _lazy_adam_rows_ref(table: torch.Tensor, exp_avg: torch.Tensor,
                        exp_avg_sq: torch.Tensor, flat_ids: torch.Tensor,
                        rows: torch.Tensor, lr: float, eps: float,
                        beta1: float, beta2: float, step: int,
                        scale: float) -> None:
    """Reference: coalesce duplicate ids, then one Adam step on the unique
    rows ONLY (== torch.optim.SparseAdam on a coalesced sparse grad), in
    fp32 and in the kernel's operation order.  ``step_size`` and the two
    ``1 - beta`` are formed in Python floats (double) and rounded to fp32
    once, where they meet the tensors."""
    uniq, inv = torch.unique(flat_ids, return_inverse=True)
    g = torch.zeros(uniq.numel(), rows.shape[1], dtype=torch.float32,
                    device=rows.device)
    g.index_add_(0, inv, rows.float())
    g.mul_(scale)
    step_size = (lr * math.sqrt(1.0 - beta2 ** step)
                 / (1.0 - beta1 ** step))
    m = exp_avg.index_select(0, uniq)
    v = exp_avg_sq.index_select(0, uniq)
    m = m + (1.0 - beta1) * (g - m)
    v = v + (1.0 - beta2) * (g * g - v)
    w = table.index_select(0, uniq) - (step_size * m) / (v.sqrt() + eps)
    exp_avg.index_copy_(0, uniq, m)
    exp_avg_sq.index_copy_(0, uniq, v)
    table.index_copy_(0, uniq, w)


class SparseSide(NamedTuple):
    """One table's side of a stateful sparse update: the rule (``"adagrad"``,
    ``"ftrl"``, ``"lazy_adam"`` or ``"rowwise_adagrad"``), the table, the
    rule's state tensors in the rule's order (``(state_sum,)``, ``(accum,
    linear)``, ``(exp_avg, exp_avg_sq)``, ``(state_row,)``), the gradient
    (deep: ``[n, dim]``; wide: per example, ``gw[i // g_div]``) and the
    rule's scalars; a rule ignores the scalars it does not have.
    ``beta1``, ``beta2`` and ``step`` are lazy Adam's: ``step`` is the count
    of updates applied to the table, this one included (>= 1)."""
    rule: str
    table: torch.Tensor
    states: Tuple[torch.Tensor, ...]
    grad: torch.Tensor
    lr: float
    eps: float = 1e-10
    l1: float = 0.0
    l2: float = 0.0
    beta1: float = 0.9
    beta2: float = 0.999
    step: int = 0


def _side_ref(side: SparseSide, flat: torch.Tensor, is_wide: bool,
              scale: float) -> None:
    """CPU reference of one side."""
    if is_wide:
        if flat.numel() == 0:
            return
        g_div = flat.numel() // side.grad.numel()
        rows = side.grad.float().reshape(-1, 1).expand(-1, g_div) \
            .reshape(-1, 1)
        tensors = [t.reshape(-1, 1) for t in (side.table, *side.states)]
    else:
        rows = side.grad.reshape(flat.numel(), -1)
        tensors = [side.table, *side.states]
    if side.rule == "ftrl":
        _ftrl_rows_ref(*tensors, flat, rows, side.lr, side.l1, side.l2,
                       scale)
    elif side.rule == "adagrad":
        _adagrad_rows_ref(*tensors, flat, rows, side.lr, side.eps, scale)
    elif side.rule == "lazy_adam":
        _lazy_adam_rows_ref(*tensors, flat, rows, side.lr, side.eps,
                            side.beta1, side.beta2, side.step, scale)
    else:
        _rowwise_adagrad_rows_ref(side.table, side.states[0], flat, rows,
                                  side.lr, side.eps, scale)


def _side_arg(side: SparseSide, acc: torch.Tensor) -> tuple:
    """A side as ``_C.emb_bwd_sparse`` takes it."""
    rule, table, states, grad, lr, eps, l1, l2, beta1, beta2, step = side
    arg = (rule, table, states, acc, grad.contiguous(), lr, eps, l1, l2)
    # lazy Adam's scalars ride behind the nine every rule has
    return arg + (beta1, beta2, step) if rule == "lazy_adam" else arg


@functools.lru_cache(maxsize=None)
def _pair_fused_ok(deep_rule: str, wide_rule: str, dim: int) -> bool:
    """``_C.sparse_pair_fused_ok``: the answer never changes, and the ops
    ask once per update."""
    return _C.sparse_pair_fused_ok(deep_rule, wide_rule, dim)


def emb_bwd_sparse(ids: torch.Tensor, *, deep: Optional[SparseSide] = None,
                   wide: Optional[SparseSide] = None, scale: float = 1.0,
                   workspace=None) -> None:
    """The stateful sparse update behind every ``emb_bwd_<rule>*`` op: on
    the rows named by ``ids``, the ``deep`` table's side, the ``[rows, 1]``
    ``wide`` table's side, or both from their shared flat ids.  For each
    unique id u, ``G = scale * sum(grad[i] for ids[i] == u)``, then the
    side's rule once per row; rows not in ``ids`` are neither read nor
    written.

    GPU: pass 1 scatter-adds into ``workspace.acc`` (/ ``wide_acc``), pass
    2 claims each touched row once and applies the rule
    (``csrc/sparse_adagrad.hip``).  A pair runs as ONE fused update (ids
    read once per pass, the winner of a deep row also applies the wide
    scalar) when ``_C.sparse_pair_fused_ok`` says there is a kernel for the
    rule pair at this ``dim`` and both gradients have one dtype (an Adagrad
    wide side also needs the deep side's ``lr``); otherwise the deep
    side runs on the workspace and the wide side on its ``wide_view()``, on
    the shared stamp across two epochs.  Pass a persistent
    :class:`SparseWorkspace` (for a pair, built with the wide table);
    without one a table-sized scratch is allocated for the call."""
    sides = [s for s in (deep, wide) if s is not None]
    for side in sides:
        if side.rule == "ftrl":
            _check_ftrl_args(side.lr, side.l1, side.l2)
        elif side.rule == "lazy_adam":
            _check_lazy_adam_args(side.lr, side.eps, side.beta1, side.beta2,
                                  side.step)
    flat = ids.reshape(-1)
    if not (ids.is_cuda or any(t.is_cuda for s in sides
                               for t in (s.table, s.grad, *s.states))):
        for side in sides:
            _side_ref(side, flat, side is wide, scale)
        return
    _require_ext()
    ws = workspace
    if ws is None:
        ws = SparseWorkspace(sides[0].table,
                             wide.table if len(sides) == 2 else None)
    if len(sides) == 1:
        side = _side_arg(sides[0], ws.acc)
        _C.emb_bwd_sparse(side if deep is not None else None,
                          side if wide is not None else None, ws.stamp,
                          flat.contiguous(), ws.next_epoch(), scale)
        return
    # An Adagrad wide side under an Adagrad or row-wise Adagrad deep side is
    # fused only at one shared lr: at two rates the pair has always taken
    # the single ops.  The kernels carry per-side scalars; lifting this is a
    # separate change.
    if (_pair_fused_ok(deep.rule, wide.rule, deep.table.shape[1])
            and deep.grad.dtype == wide.grad.dtype
            and (wide.rule != "adagrad" or wide.lr == deep.lr)):
        _C.emb_bwd_sparse(_side_arg(deep, ws.acc),
                          _side_arg(wide, ws.wide_acc), ws.stamp,
                          flat.contiguous(), ws.next_epoch(), scale)
        return
    emb_bwd_sparse(ids, deep=deep, scale=scale, workspace=ws)
    emb_bwd_sparse(ids, wide=wide, scale=scale, workspace=ws.wide_view())


def emb_bwd_adagrad(table: torch.Tensor, state_sum: torch.Tensor,
                    ids: torch.Tensor, grad: torch.Tensor, *, lr: float,
                    eps: float = 1e-10, scale: float = 1.0,
                    workspace: Optional[SparseWorkspace] = None) -> None:
    """Sparse Adagrad on the rows named by ``ids``.  For each unique id u:
    ``G = scale * sum(grad[i] for ids[i] == u)``; ``state_sum[u] += G*G``;
    ``table[u] -= lr * G / (sqrt(state_sum[u]) + eps)``.  Rows not in
    ``ids`` are neither read nor written.  ``grad`` fp32 or bf16, table
    and state fp32, any ``dim >= 1``.

    GPU: atomic scatter into ``workspace.acc`` (the existing
    ``emb_bwd_dense`` kernel), then the claim kernel updates each touched
    row exactly once (``csrc/sparse_adagrad.hip``).  Pass a persistent
    :class:`SparseWorkspace`; without one a table-sized scratch is
    allocated for the call."""
    emb_bwd_sparse(ids, deep=SparseSide("adagrad", table, (state_sum,),
                                        grad, lr, eps),
                   scale=scale, workspace=workspace)


def emb_bwd_adagrad_wide(table: torch.Tensor, state_sum: torch.Tensor,
                         ids: torch.Tensor, gw: torch.Tensor, *, lr: float,
                         eps: float = 1e-10, scale: float = 1.0,
                         workspace: Optional[SparseWorkspace] = None
                         ) -> None:
    """:func:`emb_bwd_adagrad` for the ``[rows, 1]`` wide table: the
    gradient of flat update i is the per-example ``gw[i // g_div]``,
    ``g_div = ids.numel() // gw.numel()`` (layout of
    :func:`emb_scatter_sum`)."""
    emb_bwd_sparse(ids, wide=SparseSide("adagrad", table, (state_sum,), gw,
                                        lr, eps),
                   scale=scale, workspace=workspace)


def emb_bwd_adagrad_fused_wide(table: torch.Tensor, state_sum: torch.Tensor,
                               wide_table: torch.Tensor,
                               wide_state_sum: torch.Tensor,
                               ids: torch.Tensor, grad: torch.Tensor,
                               gw: torch.Tensor, *, lr: float,
                               eps: float = 1e-10, scale: float = 1.0,
                               workspace: Optional[SparseWorkspace] = None
                               ) -> None:
    """Sparse Adagrad on BOTH CTR tables from the shared flat ids (the
    Adagrad mirror of :func:`emb_bwd_sgd_fused_wide`): the ids are read
    once per pass and the winner of a deep row also applies the wide
    scalar.  ``workspace`` must have been built with ``wide_table``.
    Shapes the fused kernels do not cover (``dim/4`` not a power of two
    <= 64, mixed grad dtypes) take the two single-table ops, sharing the
    workspace's stamp across two epochs."""
    emb_bwd_sparse(
        ids, deep=SparseSide("adagrad", table, (state_sum,), grad, lr, eps),
        wide=SparseSide("adagrad", wide_table, (wide_state_sum,), gw, lr,
                        eps),
        scale=scale, workspace=workspace)


def emb_bwd_ftrl(table: torch.Tensor, accum: torch.Tensor,
                 linear: torch.Tensor, ids: torch.Tensor,
                 grad: torch.Tensor, *, lr: float, l1: float = 0.0,
                 l2: float = 0.0, scale: float = 1.0,
                 workspace: Optional[SparseWorkspace] = None) -> None:
    """Sparse FTRL-proximal on the rows named by ``ids`` (TF ``Ftrl`` with
    ``learning_rate_power=-0.5``, no beta, no L2 shrinkage).  For each
    unique id u, ``G = scale * sum(grad[i] for ids[i] == u)`` and per
    element, with ``n = accum[u]``, ``z = linear[u]``, ``w = table[u]``::

        n' = n + G*G
        z' = z + G - (sqrt(n') - sqrt(n)) / lr * w
        w' = (sign(z') * l1 - z') / (sqrt(n') / lr + 2*l2)  if |z'| > l1
             0.0                                             otherwise

    Rows not in ``ids`` are neither read nor written (NOT a dense step
    with zero gradients); a touched row whose gradients sum to 0 is still
    recomputed from ``(z, n)``.  ``grad`` fp32 or bf16; table and both
    states fp32, any ``dim >= 1``.

    GPU: the accumulate-then-claim kernels of :func:`emb_bwd_adagrad`
    with the FTRL rule (``csrc/sparse_adagrad.hip``)."""
    emb_bwd_sparse(ids, deep=SparseSide("ftrl", table, (accum, linear),
                                        grad, lr, l1=l1, l2=l2),
                   scale=scale, workspace=workspace)


def emb_bwd_ftrl_wide(table: torch.Tensor, accum: torch.Tensor,
                      linear: torch.Tensor, ids: torch.Tensor,
                      gw: torch.Tensor, *, lr: float, l1: float = 0.0,
                      l2: float = 0.0, scale: float = 1.0,
                      workspace: Optional[SparseWorkspace] = None) -> None:
    """:func:`emb_bwd_ftrl` for the ``[rows, 1]`` wide table, with the
    ``gw[i // g_div]`` gradient layout of :func:`emb_bwd_adagrad_wide`."""
    emb_bwd_sparse(ids, wide=SparseSide("ftrl", table, (accum, linear), gw,
                                        lr, l1=l1, l2=l2),
                   scale=scale, workspace=workspace)


def emb_bwd_adagrad_ftrl_fused_wide(
        table: torch.Tensor, state_sum: torch.Tensor,
        wide_table: torch.Tensor, wide_accum: torch.Tensor,
        wide_linear: torch.Tensor, ids: torch.Tensor, grad: torch.Tensor,
        gw: torch.Tensor, *, lr: float, eps: float = 1e-10,
        wide_lr: Optional[float] = None, l1: float = 0.0, l2: float = 0.0,
        scale: float = 1.0,
        workspace: Optional[SparseWorkspace] = None) -> None:
    """The wide-and-deep recipe from the shared flat ids: sparse Adagrad
    (``lr``, ``eps``) on the deep table and sparse FTRL (``wide_lr``,
    default ``lr``; ``l1``, ``l2``) on the wide scalars, one claim per
    row for both.  ``workspace`` must have been built with ``wide_table``.
    Shapes the fused kernel does not cover take the two single-table ops
    on the shared stamp, as in :func:`emb_bwd_adagrad_fused_wide`."""
    emb_bwd_sparse(
        ids, deep=SparseSide("adagrad", table, (state_sum,), grad, lr, eps),
        wide=SparseSide("ftrl", wide_table, (wide_accum, wide_linear), gw,
                        lr if wide_lr is None else wide_lr, l1=l1, l2=l2),
        scale=scale, workspace=workspace)


def emb_bwd_ftrl_fused_wide(
        table: torch.Tensor, accum: torch.Tensor, linear: torch.Tensor,
        wide_table: torch.Tensor, wide_accum: torch.Tensor,
        wide_linear: torch.Tensor, ids: torch.Tensor, grad: torch.Tensor,
        gw: torch.Tensor, *, lr: float, wide_lr: Optional[float] = None,
        l1: float = 0.0, l2: float = 0.0, scale: float = 1.0,
        workspace: Optional[SparseWorkspace] = None) -> None:
    """Sparse FTRL on BOTH CTR tables from the shared flat ids (``l1`` and
    ``l2`` are shared; the wide table may run at its own ``wide_lr``).
    Fallback rule as in :func:`emb_bwd_adagrad_ftrl_fused_wide`."""
    emb_bwd_sparse(
        ids, deep=SparseSide("ftrl", table, (accum, linear), grad, lr,
                             l1=l1, l2=l2),
        wide=SparseSide("ftrl", wide_table, (wide_accum, wide_linear), gw,
                        lr if wide_lr is None else wide_lr, l1=l1, l2=l2),
        scale=scale, workspace=workspace)


def emb_bwd_lazy_adam(table: torch.Tensor, exp_avg: torch.Tensor,
                      exp_avg_sq: torch.Tensor, ids: torch.Tensor,
                      grad: torch.Tensor, *, lr: float, step: int,
                      beta1: float = 0.9, beta2: float = 0.999,
                      eps: float = 1e-8, scale: float = 1.0,
                      workspace: Optional[SparseWorkspace] = None) -> None:
    """Lazy (sparse) Adam on the rows named by ``ids``:
    ``torch.optim.SparseAdam`` on a coalesced gradient, TF's ``LazyAdam``.
    For each unique id u, ``G = scale * sum(grad[i] for ids[i] == u)`` and
    per element in fp32, with ``m = exp_avg[u]``, ``v = exp_avg_sq[u]``,
    ``w = table[u]``::

        m' = m + (1 - beta1) * (G - m)
        v' = v + (1 - beta2) * (G*G - v)
        w' = w - step_size * m' / (sqrt(v') + eps)
        step_size = lr * sqrt(1 - beta2**step) / (1 - beta1**step)

    ``step`` (required) is the number of updates applied to this table,
    the current one included (first call: 1); it is one count per table,
    not per row.  Rows not in ``ids`` are neither read nor written: their
    ``m`` and ``v`` do not decay (that is "lazy"); a touched row whose
    gradients sum to 0 still decays ``m`` and ``v`` and moves ``w``.
    ``eps`` sits outside the square root and is not divided by the bias
    correction, unlike :func:`fused_adam` (``torch.optim.Adam``'s form).
    ``grad`` fp32 or bf16; table and both states fp32, any ``dim >= 1``.

    GPU: the accumulate-then-claim kernels of :func:`emb_bwd_adagrad` with
    the Adam rule (``csrc/sparse_adagrad.hip``); ``step_size`` and the two
    ``1 - beta`` are formed on the host in double and rounded once."""
    emb_bwd_sparse(ids, deep=SparseSide("lazy_adam", table,
                                        (exp_avg, exp_avg_sq), grad, lr,
                                        eps, beta1=beta1, beta2=beta2,
                                        step=step),
                   scale=scale, workspace=workspace)


def emb_bwd_lazy_adam_wide(table: torch.Tensor, exp_avg: torch.Tensor,
                           exp_avg_sq: torch.Tensor, ids: torch.Tensor,
                           gw: torch.Tensor, *, lr: float, step: int,
                           beta1: float = 0.9, beta2: float = 0.999,
                           eps: float = 1e-8, scale: float = 1.0,
                           workspace: Optional[SparseWorkspace] = None
                           ) -> None:
    """:func:`emb_bwd_lazy_adam` for the ``[rows, 1]`` wide table, with the
    ``gw[i // g_div]`` gradient layout of :func:`emb_bwd_adagrad_wide`."""
    emb_bwd_sparse(ids, wide=SparseSide("lazy_adam", table,
                                        (exp_avg, exp_avg_sq), gw, lr, eps,
                                        beta1=beta1, beta2=beta2, step=step),
                   scale=scale, workspace=workspace)


def emb_bwd_lazy_adam_fused_wide(
        table: torch.Tensor, exp_avg: torch.Tensor,
        exp_avg_sq: torch.Tensor, wide_table: torch.Tensor,
        wide_exp_avg: torch.Tensor, wide_exp_avg_sq: torch.Tensor,
        ids: torch.Tensor, grad: torch.Tensor, gw: torch.Tensor, *,
        lr: float, step: int, wide_lr: Optional[float] = None,
        wide_step: Optional[int] = None, beta1: float = 0.9,
        beta2: float = 0.999, eps: float = 1e-8, scale: float = 1.0,
        workspace: Optional[SparseWorkspace] = None) -> None:
    """Lazy Adam on BOTH CTR tables from the shared flat ids (betas and
    ``eps`` are shared; the wide table may run at its own ``wide_lr`` and
    carries its own count ``wide_step``, default ``step``): one claim per
    row for both.  ``workspace`` must have been built with ``wide_table``.
    Fallback rule as in :func:`emb_bwd_adagrad_fused_wide`."""
    emb_bwd_sparse(
        ids, deep=SparseSide("lazy_adam", table, (exp_avg, exp_avg_sq), grad,
                             lr, eps, beta1=beta1, beta2=beta2, step=step),
        wide=SparseSide("lazy_adam", wide_table,
                        (wide_exp_avg, wide_exp_avg_sq), gw,
                        lr if wide_lr is None else wide_lr, eps, beta1=beta1,
                        beta2=beta2,
                        step=step if wide_step is None else wide_step),
        scale=scale, workspace=workspace)


def emb_bwd_lazy_adam_ftrl_fused_wide(
        table: torch.Tensor, exp_avg: torch.Tensor,
        exp_avg_sq: torch.Tensor, wide_table: torch.Tensor,
        wide_accum: torch.Tensor, wide_linear: torch.Tensor,
        ids: torch.Tensor, grad: torch.Tensor, gw: torch.Tensor, *,
        lr: float, step: int, beta1: float = 0.9, beta2: float = 0.999,
        eps: float = 1e-8, wide_lr: Optional[float] = None, l1: float = 0.0,
        l2: float = 0.0, scale: float = 1.0,
        workspace: Optional[SparseWorkspace] = None) -> None:
    """Lazy Adam (``lr``, betas, ``eps``, ``step``) on the deep table and
    sparse FTRL (``wide_lr``, default ``lr``; ``l1``, ``l2``) on the wide
    scalars from the shared flat ids, one claim per row for both.
    Fallback rule as in :func:`emb_bwd_adagrad_ftrl_fused_wide`."""
    emb_bwd_sparse(
        ids, deep=SparseSide("lazy_adam", table, (exp_avg, exp_avg_sq), grad,
                             lr, eps, beta1=beta1, beta2=beta2, step=step),
        wide=SparseSide("ftrl", wide_table, (wide_accum, wide_linear), gw,
                        lr if wide_lr is None else wide_lr, l1=l1, l2=l2),
        scale=scale, workspace=workspace)


def emb_bwd_rowwise_adagrad(table: torch.Tensor, state_row: torch.Tensor,
                            ids: torch.Tensor, grad: torch.Tensor, *,
                            lr: float, eps: float = 1e-10,
                            scale: float = 1.0,
                            workspace: Optional[SparseWorkspace] = None
                            ) -> None:
    """Row-wise sparse Adagrad on the rows named by ``ids``: ONE fp32
    accumulator value per row (``state_row``, contiguous ``[rows]``), the
    running mean of the row's squared gradient, in place of
    :func:`emb_bwd_adagrad`'s table-shaped ``state_sum``.  For each
    unique id u, in fp32::

        G[u, :]       = scale * sum(grad[i] for ids[i] == u)
        state_row[u] += (sum_c G[u, c]^2) / dim
        table[u, :]  -= lr * G[u, :] / (sqrt(state_row[u]) + eps)

    with the NEW ``state_row[u]`` in the last line.  Rows not in ``ids``
    are neither read nor written.  ``grad`` fp32 or bf16, table and state
    fp32, any ``dim >= 1`` (``dim == 1`` is element-wise Adagrad).

    GPU: pass 1 of :func:`emb_bwd_adagrad` into ``workspace.acc``, then
    the row-wise claim kernels of ``csrc/sparse_adagrad.hip``."""
    emb_bwd_sparse(ids, deep=SparseSide("rowwise_adagrad", table,
                                        (state_row,), grad, lr, eps),
                   scale=scale, workspace=workspace)


def emb_bwd_rowwise_adagrad_fused_wide(
        table: torch.Tensor, state_row: torch.Tensor,
        wide_table: torch.Tensor, wide_state_sum: torch.Tensor,
        ids: torch.Tensor, grad: torch.Tensor, gw: torch.Tensor, *,
        lr: float, eps: float = 1e-10, scale: float = 1.0,
        workspace: Optional[SparseWorkspace] = None) -> None:
    """Row-wise sparse Adagrad on the deep table and sparse Adagrad on the
    wide scalars from the shared flat ids, at one ``lr`` and ``eps``: the
    winner of a deep row also applies the wide scalar.  ``workspace`` must
    have been built with ``wide_table``.  Shapes the fused kernel does not
    cover take the two single-table ops on the shared stamp, as in
    :func:`emb_bwd_adagrad_fused_wide`."""
    emb_bwd_sparse(
        ids, deep=SparseSide("rowwise_adagrad", table, (state_row,), grad,
                             lr, eps),
        wide=SparseSide("adagrad", wide_table, (wide_state_sum,), gw, lr,
                        eps),
        scale=scale, workspace=workspace)


def emb_bwd_rowwise_adagrad_ftrl_fused_wide(
        table: torch.Tensor, state_row: torch.Tensor,
        wide_table: torch.Tensor, wide_accum: torch.Tensor,
        wide_linear: torch.Tensor, ids: torch.Tensor, grad: torch.Tensor,
        gw: torch.Tensor, *, lr: float, eps: float = 1e-10,
        wide_lr: Optional[float] = None, l1: float = 0.0, l2: float = 0.0,
        scale: float = 1.0,
        workspace: Optional[SparseWorkspace] = None) -> None:
    """The wide-and-deep recipe with a row-wise deep table: row-wise
    sparse Adagrad (``lr``, ``eps``) on the deep table and sparse FTRL
    (``wide_lr``, default ``lr``; ``l1``, ``l2``) on the wide scalars, one
    claim per row for both.  Fallback rule as in
    :func:`emb_bwd_rowwise_adagrad_fused_wide`."""
    emb_bwd_sparse(
        ids, deep=SparseSide("rowwise_adagrad", table, (state_row,), grad,
                             lr, eps),
        wide=SparseSide("ftrl", wide_table, (wide_accum, wide_linear), gw,
                        lr if wide_lr is None else wide_lr, l1=l1, l2=l2),
        scale=scale, workspace=workspace)


# ---- elementwise -----------------------------------------------------------

def bias_relu_fwd(x: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    if _on_gpu(x, bias):
        _require_ext()
        return _C.bias_relu_fwd(x.contiguous(), bias.contiguous())
    return torch.relu(x + bias)


def bias_relu_bwd(dy: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    if _on_gpu(dy, y):
        _require_ext()
        return _C.bias_relu_bwd(dy.contiguous(), y.contiguous())
    return dy * (y > 0).to(dy.dtype)


def convert_scaled(src: torch.Tensor, dst: torch.Tensor,
                   scale: float = 1.0) -> None:
    if _on_gpu(src, dst):
        _require_ext()
        _C.convert_scaled(src, dst, scale)
        return
    dst.copy_((src.float() * scale).to(dst.dtype))


def emb_fwd_into(table: torch.Tensor, ids: torch.Tensor,
                 out: torch.Tensor, col_offset: int) -> None:
    """Gather row (b,f) into out[b, col_offset + f*dim : +dim]."""
    if _on_gpu(table, ids, out):
        _require_ext()
        _C.emb_fwd_into(table, ids.reshape(-1).contiguous(), out,
                        col_offset)
        return
    batch = out.shape[0]
    f = ids.numel() // batch
    dim = table.shape[1]
    gathered = table.index_select(0, ids.reshape(-1)).reshape(
        batch, f * dim)
    out[:, col_offset:col_offset + f * dim] = gathered.to(out.dtype)


def emb_gather_sum(table: torch.Tensor, ids: torch.Tensor,
                   out_bf16: bool = False) -> torch.Tensor:
    """out[b] = sum_f table[ids[b, f], 0] for a scalar (dim-1) table."""
    batch = ids.shape[0]
    if _on_gpu(table, ids):
        _require_ext()
        return _C.emb_gather_sum(table, ids.reshape(-1).contiguous(),
                                 batch, out_bf16)
    out = table.reshape(-1).index_select(
        0, ids.reshape(-1)).reshape(batch, -1).sum(dim=1)
    return out.to(torch.bfloat16) if out_bf16 else out


def _env_switch_on(name: str) -> bool:
    """A default-on A/B switch: only an empty value or "0" turns it off."""
    return os.environ.get(name, "1") not in ("", "0")


def fused_lookup_enabled() -> bool:
    """MIYARN_FUSED_LOOKUP=0 restores the separate forward ops (offset
    add, ``emb_fwd_into``, ``emb_gather_sum``, two fills) and the scatter
    from pre-added flat ids."""
    return _env_switch_on("MIYARN_FUSED_LOOKUP")


def emb_lookup_fused_covers(table: torch.Tensor, ids: torch.Tensor,
                            dense: Optional[torch.Tensor],
                            out: torch.Tensor, col_offset: int) -> bool:
    """True when :func:`emb_lookup_fused` runs as ONE kernel for these
    operands (GPU, ``dim``, ``col_offset`` and the row stride of ``out``
    multiples of 4, ``n_dense <= col_offset``, the feature count within
    the kernel's LDS array)."""
    if not (HAVE_EXT and table.is_cuda and ids.is_cuda and out.is_cuda
            and ids.dim() == 2 and out.dim() == 2 and out.is_contiguous()
            and out.dtype in (torch.bfloat16, torch.float32)):
        return False
    n_dense = 0
    if dense is not None:
        if not (dense.is_cuda and dense.dim() == 2
                and dense.dtype == out.dtype):
            return False
        n_dense = dense.shape[1]
    return _C.emb_lookup_fused_ok(table.shape[1], ids.shape[1], n_dense,
                                  col_offset, out.shape[1])


def emb_lookup_fused(table: torch.Tensor, wide_table: torch.Tensor,
                     ids: torch.Tensor, offsets: torch.Tensor,
                     dense: Optional[torch.Tensor], out: torch.Tensor,
                     col_offset: int) -> torch.Tensor:
    """The single-GPU sparse forward from the RAW ids ``[B, F]``::

        out[b, col_offset + f*dim : +dim] = table[ids[b, f] + offsets[f]]
        out[b, :n_dense] = dense[b];  out[b, n_dense:col_offset] = 0
        wide[b] = sum_f wide_table[ids[b, f] + offsets[f]]   (returned)

    ``dense`` is ``[B, n_dense]`` in ``out``'s dtype (or None); ``wide``
    comes back in ``out``'s dtype, summed in fp32 in the order
    ``f = 0 .. F-1`` exactly as :func:`emb_gather_sum` does.  One HIP
    kernel where :func:`emb_lookup_fused_covers` holds; every other case,
    the CPU included, is the composition of the separate ops, so results
    are the same bits either way."""
    b, f = ids.shape
    dim = table.shape[1]
    if emb_lookup_fused_covers(table, ids, dense, out, col_offset):
        return _C.emb_lookup_fused(
            table, wide_table.reshape(-1), ids.contiguous(), offsets,
            None if dense is None else dense.contiguous(), out, col_offset)
    if _on_gpu(table, ids, out):
        _require_ext()
    n_dense = 0
    if dense is not None:
        n_dense = dense.shape[1]
        out[:, :n_dense] = dense
    if col_offset > n_dense:
        out[:, n_dense:col_offset] = 0
    flat = (ids + offsets.unsqueeze(0)).reshape(-1)
    out_bf16 = out.dtype == torch.bfloat16
    if not _on_gpu(table, ids, out) or (
            dim % 4 == 0 and col_offset % 4 == 0
            and out.shape[1] % 4 == 0 and out.is_contiguous()):
        emb_fwd_into(table, flat, out, col_offset)
    else:  # shapes emb_fwd_into does not take: gather, then place
        rows = emb_fwd(table, flat, out_bf16)
        out[:, col_offset:col_offset + f * dim] = \
            rows.reshape(b, f * dim).to(out.dtype)
    return emb_gather_sum(wide_table, flat.reshape(b, f), out_bf16)


def emb_scatter_sum(table: torch.Tensor, ids: torch.Tensor,
                    grad: torch.Tensor, alpha: float) -> None:
    """table[ids[b, f], 0] += alpha * grad[b] (gather-sum backward)."""
    if _on_gpu(table, ids, grad):
        _require_ext()
        _C.emb_scatter_sum(table, ids.reshape(-1).contiguous(),
                           grad.contiguous(), alpha)
        return
    f = ids.reshape(grad.numel(), -1).shape[1]
    expanded = grad.float().reshape(-1, 1).expand(-1, f).reshape(-1)
    table.reshape(-1).index_add_(0, ids.reshape(-1), expanded,
                                 alpha=alpha)


# ---- multi-hot embedding bags ----------------------------------------------

COMBINERS = ("sum", "mean", "sqrtn")


def _check_bags(ids: torch.Tensor, bag_offsets: torch.Tensor,
                n_features: int, weights: Optional[torch.Tensor],
                nnz: int) -> int:
    """Shape checks shared by the CPU and HIP paths (nothing here waits
    for a device); returns the number of examples ``B``."""
    if n_features < 1:
        raise ValueError(f"n_features must be >= 1, got {n_features!r}")
    if bag_offsets.dtype != torch.int64 or bag_offsets.dim() != 1:
        raise ValueError("bag_offsets must be a 1-D int64 tensor")
    n_bags = bag_offsets.numel() - 1
    if n_bags < 0 or n_bags % n_features:
        raise ValueError(
            f"bag_offsets must have B * n_features + 1 entries "
            f"(n_features={n_features}), got {bag_offsets.numel()}")
    if ids is not None and (ids.dtype != torch.int64 or ids.dim() != 1):
        raise ValueError("ids must be the flat 1-D int64 [nnz] array")
    if weights is not None:
        if weights.dtype != torch.float32:
            raise ValueError("weights must be fp32")
        if weights.numel() != nnz:
            raise ValueError(f"weights must have one entry per id: {nnz}, "
                             f"got {weights.numel()}")
    return n_bags // n_features


def _debug_check_bags(bag_offsets: torch.Tensor, nnz: int) -> None:
    """MIYARN_DEBUG_BOUNDS=1 on the CPU path (the HIP path checks the same
    in C++): ``bag_offsets`` starts at 0, ends at ``nnz`` and never
    decreases."""
    if bag_offsets[0].item() != 0 or bag_offsets[-1].item() != nnz:
        raise RuntimeError(
            f"bag_offsets must start at 0 and end at nnz = {nnz}, got "
            f"[{bag_offsets[0].item()} .. {bag_offsets[-1].item()}] "
            "(MIYARN_DEBUG_BOUNDS check)")
    if bag_offsets.numel() > 1 and (bag_offsets[1:]
                                    - bag_offsets[:-1]).min().item() < 0:
        raise RuntimeError("bag_offsets must be non-decreasing "
                           "(MIYARN_DEBUG_BOUNDS check)")


def _bounds_debug() -> bool:
    return os.environ.get("MIYARN_DEBUG_BOUNDS", "") not in ("", "0")


def _bag_lengths(bag_offsets: torch.Tensor):
    return bag_offsets[:-1], bag_offsets[1:] - bag_offsets[:-1]


def _emb_bag_fwd_ref(table, ids, bag_offsets, n_features, offsets, weights,
                     combiner, out, col_offset):
    """The definition on the CPU, fp32, in the kernel's operation order:
    step j adds entry j of every bag that has one, so each bag's sum runs
    in ascending entry order.  ``fmaf`` is a float64 multiply-add rounded
    to fp32 (the product is exact in float64)."""
    n_bags = bag_offsets.numel() - 1
    dim = table.shape[1]
    lo, lens = _bag_lengths(bag_offsets)
    if offsets is not None:
        feat = torch.arange(n_bags, device=ids.device) % n_features
        flat = ids + torch.repeat_interleave(offsets[feat], lens)
    else:
        flat = ids
    if _bounds_debug() and flat.numel():
        mn, mx = flat.min().item(), flat.max().item()
        if mn < 0 or mx >= table.shape[0]:
            raise RuntimeError(
                f"embedding ids out of range: [{mn}, {mx}] vs table rows "
                f"{table.shape[0]} (MIYARN_DEBUG_BOUNDS check)")
    acc = torch.zeros(n_bags, dim, dtype=torch.float32, device=table.device)
    den = (torch.zeros(n_bags, dtype=torch.float32, device=table.device)
           if weights is not None else lens.float())
    active = torch.nonzero(lens > 0).reshape(-1)
    j = 0
    while active.numel():
        pos = lo[active] + j
        rows = table.index_select(0, flat[pos])
        if weights is None:
            acc[active] = acc[active] + rows
        else:
            w = weights[pos]
            acc[active] = (w.double().unsqueeze(1) * rows.double()
                           + acc[active].double()).float()
            if combiner == "mean":
                den[active] = den[active] + w
            elif combiner == "sqrtn":
                den[active] = den[active] + w * w
        j += 1
        active = active[lens[active] > j]
    if combiner == "sum":
        scale = (lens > 0).float()
    else:
        ok = (lens > 0) & (den != 0)
        d = torch.where(ok, den, torch.ones_like(den))
        if combiner == "sqrtn":  # through float64, rounded once
            inv = (1.0 / d.double().sqrt()).float()
        else:  # tensor / tensor: a correctly rounded fp32 division
            inv = torch.ones_like(d) / d
        scale = torch.where(ok, inv, torch.zeros_like(inv))
        acc = acc * scale.unsqueeze(1)
    out[:, col_offset:col_offset + n_features * dim] = \
        acc.reshape(-1, n_features * dim).to(out.dtype)
    return scale, flat


def emb_bag_fwd(table: torch.Tensor, ids: torch.Tensor,
                bag_offsets: torch.Tensor, n_features: int, *,
                offsets: Optional[torch.Tensor] = None,
                weights: Optional[torch.Tensor] = None,
                combiner: str = "sum", out: Optional[torch.Tensor] = None,
                col_offset: int = 0, out_bf16: bool = False):
    """Pooled multi-hot lookup from CSR bags; returns ``(out, bag_scale,
    flat_ids)``.

    ``table [rows, dim]`` fp32; ``ids [nnz]`` int64, the raw per-feature
    ids; ``bag_offsets [B * n_features + 1]`` int64, non-decreasing from 0
    to ``nnz``.  Bag ``k = b * F + f`` holds entries ``bag_offsets[k] ..
    bag_offsets[k+1] - 1`` and entry ``i`` names row ``ids[i] +
    offsets[k % F]`` (``offsets [F]`` int64, optional).  ``weights [nnz]``
    fp32 are inputs: no gradient flows to them.  Per bag and column, in
    fp32::

        acc = 0;  for i ascending:  acc = acc + row_i[c]            (no weights)
                                    acc = fmaf(w_i, row_i[c], acc)  (weights)
        out[b, col_offset + f*dim + c] = acc * bag_scale[k]

    rounded once if ``out`` is bf16.  ``bag_scale`` (fp32, returned for
    the backward) is 1 for ``"sum"``; ``1/len`` or ``1/sum w`` for
    ``"mean"``; ``1/sqrt(len)`` or ``1/sqrt(sum w^2)`` for ``"sqrtn"``,
    the sums in fp32 in entry order (``w * w`` rounded before it is
    added; ``1/sqrt`` of the fp32 sum is taken in float64 and rounded
    once, which keeps the scale within 1 ulp).  An empty bag, or a zero denominator,
    has ``bag_scale`` 0 and an all-zero output: the convention of TF's
    ``safe_embedding_lookup_sparse`` for empty bags, extended to a zero
    weight sum, where TF would divide by zero.  The sum order is ascending
    position in the bag and nothing else, so two calls agree to the bit and
    a bag gives the same bits wherever it sits in the batch.

    ``out`` (contiguous 2-D fp32/bf16) receives the ``[B, F * dim]`` block
    at ``col_offset`` and keeps its other columns; ``out=None`` allocates
    ``[B, F * dim]`` (bf16 with ``out_bf16``).  ``flat_ids`` is ``ids``
    itself without ``offsets``.  ``nnz == 0`` is legal.  A long bag is
    walked serially by one lane group (not tuned).  MIYARN_DEBUG_BOUNDS=1
    also validates ``bag_offsets`` and the id range (waits for the
    device)."""
    if combiner not in COMBINERS:
        raise ValueError(
            f"combiner must be one of {COMBINERS}, got {combiner!r}")
    batch = _check_bags(ids, bag_offsets, n_features, weights, ids.numel())
    if offsets is not None and offsets.numel() != n_features:
        raise ValueError("offsets must be int64 [n_features]")
    dim = table.shape[1]
    if out is None:
        out = torch.empty(
            batch, n_features * dim, device=table.device,
            dtype=torch.bfloat16 if out_bf16 else torch.float32)
        col_offset = 0
    if (out.dim() != 2 or out.shape[0] != batch or col_offset < 0
            or col_offset + n_features * dim > out.shape[1]):
        raise ValueError(
            f"the [{batch}, {n_features * dim}] block at column "
            f"{col_offset} does not fit out {tuple(out.shape)}")
    if _on_gpu(table, ids, out):
        _require_ext()
        bag_scale, flat = _C.emb_bag_fwd(table, ids, bag_offsets,
                                         n_features, offsets, weights,
                                         combiner, out, col_offset)
        return out, bag_scale, flat
    if _bounds_debug():
        _debug_check_bags(bag_offsets, ids.numel())
    bag_scale, flat = _emb_bag_fwd_ref(table, ids, bag_offsets, n_features,
                                       offsets, weights, combiner, out,
                                       col_offset)
    return out, bag_scale, flat


def emb_bag_bwd_rows(grad_out: torch.Tensor, bag_offsets: torch.Tensor,
                     bag_scale: torch.Tensor, dim: int, n_features: int, *,
                     weights: Optional[torch.Tensor] = None,
                     col_offset: int = 0,
                     nnz: Optional[int] = None) -> torch.Tensor:
    """The backward of :func:`emb_bag_fwd` as update rows: for entry ``i``
    of bag ``k = (b, f)``::

        s_i = bag_scale[k]  (* w_i with weights: one fp32 multiply)
        grad_rows[i, c] = grad_out[b, col_offset + f*dim + c] * s_i

    rounded to ``grad_out``'s dtype (fp32 or bf16); ``"sum"`` without
    weights is a copy, bit for bit.  ``grad_out`` is the whole ``[B,
    cols]`` gradient, read in place at ``col_offset`` (rows may lie a
    stride apart).  With ``flat_ids`` of the forward, ``grad_rows [nnz,
    dim]`` is the update list every sparse update op takes; an id that
    appears twice in a bag appears twice in it, and the update ops sum
    it.  ``nnz`` (``ids.numel()`` of the forward) sizes the result; without
    it and without ``weights`` the GPU path reads ``bag_offsets[-1]`` back
    from the device, the only wait in these two ops."""
    if nnz is None and weights is not None:
        nnz = int(weights.numel())
    batch = _check_bags(None, bag_offsets, n_features, weights, nnz)
    if bag_scale.numel() != batch * n_features:
        raise ValueError("bag_scale must have one entry per bag")
    if (grad_out.dim() != 2 or grad_out.shape[0] != batch or col_offset < 0
            or col_offset + n_features * dim > grad_out.shape[1]):
        raise ValueError(
            f"the [{batch}, {n_features * dim}] block at column "
            f"{col_offset} does not fit grad_out {tuple(grad_out.shape)}")
    if _on_gpu(grad_out, bag_offsets, bag_scale):
        _require_ext()
        if nnz is None:
            nnz = int(bag_offsets[-1].item())
        if grad_out.stride(1) != 1 or grad_out.stride(0) < grad_out.shape[1]:
            grad_out = grad_out.contiguous()
        return _C.emb_bag_bwd_rows(grad_out, bag_offsets, bag_scale, dim,
                                   n_features, nnz, weights, col_offset)
    _, lens = _bag_lengths(bag_offsets)
    n_bags = batch * n_features
    if _bounds_debug():
        _debug_check_bags(bag_offsets, int(lens.sum().item()))
    bag = torch.repeat_interleave(torch.arange(n_bags), lens)
    s = bag_scale[bag]
    if weights is not None:
        s = s * weights
    g = grad_out[:, col_offset:col_offset + n_features * dim] \
        .reshape(n_bags, dim)[bag]
    return (g.float() * s.unsqueeze(1)).to(grad_out.dtype)


class EmbeddingBagFn(torch.autograd.Function):
    """Pooled multi-hot lookup (:func:`emb_bag_fwd`) whose backward appends
    ``(flat_ids [nnz], grad_rows [nnz, dim])`` to ``sink``: the update list
    the sparse update ops consume.  With ``dense`` the result is the MLP
    input ``[B, col_offset + F * dim]`` in one buffer: dense columns first,
    zeros up to ``col_offset``, the pooled block in the slice.  ``wrap``
    makes the sink entry from the ``(flat_ids, grad_rows)`` pair (``tuple``,
    or a module's marker type).  All twelve arguments are positional."""

    @staticmethod
    def forward(ctx, table, ids, bag_offsets, n_features, offsets, weights,
                combiner, out_bf16, sink, dense, col_offset, wrap):
        dim = table.shape[1]
        batch = (bag_offsets.numel() - 1) // n_features
        out = None
        if dense is not None or col_offset:
            out = torch.empty(
                batch, col_offset + n_features * dim, device=table.device,
                dtype=torch.bfloat16 if out_bf16 else torch.float32)
            n_dense = 0
            if dense is not None:
                n_dense = dense.shape[1]
                out[:, :n_dense] = dense.to(out.dtype)
            out[:, n_dense:col_offset] = 0
        out, bag_scale, flat_ids = emb_bag_fwd(
            table.detach(), ids, bag_offsets, n_features, offsets=offsets,
            weights=weights, combiner=combiner, out=out,
            col_offset=col_offset, out_bf16=out_bf16)
        ctx.sink, ctx.wrap = sink, wrap
        ctx.dims = (dim, n_features, col_offset, ids.numel())
        ctx.weights = weights
        ctx.save_for_backward(bag_offsets, bag_scale, flat_ids)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        bag_offsets, bag_scale, flat_ids = ctx.saved_tensors
        dim, n_features, col_offset, nnz = ctx.dims
        rows = emb_bag_bwd_rows(grad_out, bag_offsets, bag_scale, dim,
                                n_features, weights=ctx.weights,
                                col_offset=col_offset, nnz=nnz)
        ctx.sink.append(ctx.wrap((flat_ids, rows)))
        return (None,) * 12


def col_reduce_dot(x: torch.Tensor, dy: torch.Tensor) -> torch.Tensor:
    """dw[m] = sum_b dy[b] * x[b, m] (fp32 result)."""
    if _on_gpu(x, dy):
        _require_ext()
        return _C.col_reduce_dot(x.contiguous(), dy.contiguous())
    return (x.float() * dy.float().unsqueeze(1)).sum(dim=0)


def fused_head_grads_enabled() -> bool:
    """MIYARN_FUSED_HEAD_GRADS=0 restores the separate kernels for a
    single-logit head's own gradients: ``col_reduce_dot`` and its cast for
    the weight, ``dl.sum()`` and its cast for the bias."""
    return _env_switch_on("MIYARN_FUSED_HEAD_GRADS")


def col_reduce_dot_sum(x: torch.Tensor, dy: torch.Tensor,
                       out_dtype: torch.dtype = torch.float32):
    """``(dw, db)`` of a single-logit head from ONE pass over ``x``:
    ``dw[m] = sum_b dy[b] * x[b, m]`` as :func:`col_reduce_dot` computes
    it and ``db [1] = sum_b dy[b]``, both summed in fp32 and stored as
    ``out_dtype`` (fp32 or bf16, rounded once).  On the GPU the two are
    views of one buffer."""
    if _on_gpu(x, dy):
        _require_ext()
        if out_dtype in (torch.float32, torch.bfloat16):
            dw, db = _C.col_reduce_dot_sum(x.contiguous(), dy.contiguous(),
                                           out_dtype == torch.bfloat16)
            return dw, db
        dw, db = _C.col_reduce_dot_sum(x.contiguous(), dy.contiguous(),
                                       False)
        return dw.to(out_dtype), db.to(out_dtype)
    dw = (x.float() * dy.float().unsqueeze(1)).sum(dim=0)
    db = dy.float().sum().reshape(1)
    return dw.to(out_dtype), db.to(out_dtype)


def row_dot(x: torch.Tensor, w: torch.Tensor,
            bias: "torch.Tensor | None" = None) -> torch.Tensor:
    """y[b] = x[b] . w (+ bias): streaming GEMV for the single-logit
    head forward (hipBLASLt's M=1 bias-GEMV ran at ~175 GB/s)."""
    if _on_gpu(x, w) and x.size(1) % 4 == 0 and x.size(1) <= 512:
        _require_ext()
        return _C.row_dot(x.contiguous(), w.contiguous(), bias)
    y = x @ w
    return y if bias is None else y + bias


def gemm_bt(a: torch.Tensor, b: torch.Tensor,
            bias: "torch.Tensor | None" = None,
            relu: bool = False) -> torch.Tensor:
    """C[M, N] = A[M, K] @ B[N, K]^T (nn.Linear forward form), optional
    fused bias+ReLU epilogue. Both operands K-major bf16 on GPU."""
    if _on_gpu(a, b):
        _require_ext()
        return _C.gemm_bt(a.contiguous(), b.contiguous(), bias, relu)
    out = a.float() @ b.float().t()
    if bias is not None:
        out = out + bias.float()
    if relu:
        out = torch.relu(out)
    return out.to(a.dtype)


class ScalarHeadFn(torch.autograd.Function):
    """y[b] = x[b].w + bias for a single-logit head; the wgrad runs as a
    streaming column reduction instead of hipBLASLt's M=1 GEMM
    (187 us -> ~15 us measured at 65536x256)."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        ctx.save_for_backward(x, weight)
        if _on_gpu(x, weight) and x.size(1) % 4 == 0 \
                and x.size(1) <= 512 and bias.numel() == 1:
            _require_ext()
            return _C.row_dot(x.contiguous(), weight.contiguous(),
                              bias.reshape(1))
        return x @ weight + bias

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        dy = dy.contiguous()
        dx = dw = db = None
        if ctx.needs_input_grad[0]:  # input data (wide head) needs no dx
            dx = dy.unsqueeze(1) * weight.unsqueeze(0)
        if ctx.needs_input_grad[1] and ctx.needs_input_grad[2] \
                and _on_gpu(x, dy) and x.dtype == dy.dtype \
                and fused_head_grads_enabled():
            dw, db = col_reduce_dot_sum(x, dy, weight.dtype)
            return dx, dw, db
        if ctx.needs_input_grad[1]:
            dw = col_reduce_dot(x, dy).to(weight.dtype)
        if ctx.needs_input_grad[2]:
            db = dy.sum().reshape(1).to(weight.dtype)
        return dx, dw, db


class BCEHeadFn(torch.autograd.Function):
    """Per-example BCEWithLogits over logits = deep + wide + dhead,
    fused into one kernel pair (saves the two adds, the fp32 cast, and
    torch's separate loss fwd/bwd elementwise kernels)."""

    @staticmethod
    def forward(ctx, deep, wide, dhead, labels):
        if deep.is_cuda and HAVE_EXT and deep.dtype == torch.bfloat16 \
                and wide.dtype == torch.bfloat16 \
                and dhead.dtype == torch.bfloat16:
            loss, sig = _C.bce_head_fwd(
                deep.contiguous(), wide.contiguous(), dhead.contiguous(),
                labels.contiguous().float())
        else:
            z = (deep.float() + wide.float() + dhead.float())
            labels = labels.float()
            loss = torch.nn.functional.binary_cross_entropy_with_logits(
                z, labels, reduction="none")
            sig = torch.sigmoid(z).to(deep.dtype)
        ctx.save_for_backward(sig, labels)
        ctx.dtype = deep.dtype
        return loss

    @staticmethod
    def backward(ctx, g):
        sig, labels = ctx.saved_tensors
        if sig.is_cuda and HAVE_EXT and sig.dtype == torch.bfloat16:
            dl = _C.bce_head_bwd(sig, labels.contiguous().float(),
                                 g.contiguous().float())
        else:
            dl = ((sig.float() - labels.float()) * g.float()).to(ctx.dtype)
        return dl, dl, dl, None


def bce_head_loss(deep: torch.Tensor, wide: torch.Tensor,
                  dhead: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
    """Mean BCEWithLogits over the fused 3-part head."""
    return BCEHeadFn.apply(deep, wide, dhead, labels).mean()


class BiasReLU(torch.autograd.Function):
    """Autograd wrapper for the fused bias+ReLU epilogue (backward fuses
    the dbias reduction into the dx kernel on GPU)."""

    @staticmethod
    def forward(ctx, x, bias):
        y = bias_relu_fwd(x, bias)
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        if dy.is_cuda and HAVE_EXT and y.size(-1) % 4 == 0 \
                and y.size(-1) <= 8192:
            # v3 fused kernel: atomic-free per-block column partials +
            # one tiny reduce (earlier atomic/LDS variants measured
            # slower than the separate path; see micro_elementwise.py).
            dx, dbias = _C.bias_relu_bwd_db(
                dy.contiguous(), y.contiguous(),
                dy.dtype == torch.bfloat16)
            return dx, dbias.to(dy.dtype)
        dx = bias_relu_bwd(dy.contiguous(), y)
        dims = tuple(range(dx.dim() - 1))
        dbias = dx.sum(dim=dims)
        return dx, dbias


def bias_relu(x: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    return BiasReLU.apply(x, bias)


def _custom_wgrad_kernel(dz: torch.Tensor, x: torch.Tensor):
    """Pick the split-K MFMA wgrad variant for this shape, or None to use
    hipBLASLt.  Measured (micro_gemm.py, B=65536): 256^2 tiles reach
    312/359 TF on the 1024x432 / 512x1024 layers (hipBLASLt in-context ran
    them at ~207 us each); 128^2 tiles win the small 256x512 layer
    (94 us vs ~142-190).  ``MIYARN_WGRAD=regstage`` keeps this choice and
    makes :func:`_linear_wgrad` ask the kernel for its register-staged
    k-loop (the control of the LDS-DMA staging; same bits)."""
    if os.environ.get("MIYARN_WGRAD") == "lib":
        return None  # A/B escape hatch: force hipBLASLt
    if not (dz.is_cuda and HAVE_EXT):
        return None
    if dz.dtype != torch.bfloat16 or x.dtype != torch.bfloat16:
        return None
    n, m = dz.size(1), x.size(1)
    if m % 8 != 0 or dz.size(0) % 64 != 0:
        return None
    if n % 256 == 0 and n * m > 256 * 512:
        return _C.wgrad_nt256
    if n % 128 == 0 and n * m <= 256 * 512:
        return _C.wgrad_nt128
    return None


def _fused_dgrad_shape_routed(k: int, n: int) -> bool:
    """Whether a hidden layer's dgrad of this shape (``dz_next [B, k]``,
    weight ``[k, n]``) runs as ``_C.dgrad_drelu`` inside
    :class:`MLPHeadFn`.  A shape is routed only if the fused kernel's
    median lies below that of library dgrad + ``bias_relu_bwd_db`` by more
    than the larger min..max spread of the two.  Measured
    (``micro_gemm.py --dgrad-fused``, B=65536, median of 7 windows of 20
    calls (min .. max), us; two boxes):

    ===========  =========  =====================  =====================
    k -> n       lib dgrad  lib + bias_relu_bwd    dgrad_drelu
    ===========  =========  =====================  =====================
    256 -> 512   32.1       79.8 (78.5 .. 80.5)    52.8 (51.9 .. 53.9)
    256 -> 512   32.4       81.5 (80.4 .. 82.5)    54.9 (53.6 .. 57.0)
    512 -> 1024  85.4       150.6 (149.1 .. 153.8)  133.3 (131.2 .. 135.0)
    512 -> 1024  85.5       155.4 (155.2 .. 156.8)  137.2 (132.7 .. 141.9)
    ===========  =========  =====================  =====================

    Both pass: 27 us against a spread of 3.4, 17-18 us against 9.2.  The
    larger shape passes only at the kernel's present 164 VGPRs (three
    blocks per CU); at two blocks per CU it measured level with the
    library pair (``profiles/r09_dgrad_drelu.md``).  Other shapes have not
    been measured and stay on the library."""
    return (k, n) in _FUSED_DGRAD_SHAPES


_FUSED_DGRAD_SHAPES = frozenset({(256, 512), (512, 1024)})


def _custom_fwd_ok(x: torch.Tensor, weight: torch.Tensor,
                   bias: torch.Tensor) -> bool:
    """True when gemm_bt should fuse the whole forward (GEMM + bias +
    ReLU in one kernel).  OPT-IN (MIYARN_FWD=custom): measured on MI355X
    the fused kernel runs at 361-613 TF on the MLP forward shapes while
    hipBLASLt + the separate bias_relu kernel reach 444-831 TF combined —
    with only 7-16 K-tile iterations the software pipeline never hits the
    steady state the wgrad kernels reach over B=65536 (scripts/
    micro_gemm.py --fwd)."""
    if os.environ.get("MIYARN_FWD") != "custom":
        return False
    if not (x.is_cuda and HAVE_EXT):
        return False
    if x.dtype != torch.bfloat16 or weight.dtype != torch.bfloat16 \
            or bias.dtype != torch.bfloat16:
        return False
    if x.dim() != 2 or not x.is_contiguous() or not weight.is_contiguous():
        return False
    m, k = x.shape
    return m % 256 == 0 and k % 16 == 0 and weight.size(0) % 16 == 0


def _lt_fwd_ok(x, weight, bias) -> bool:
    """Fuse bias+ReLU into the hipBLASLt GEMM epilogue (lt_linear): one
    library call, no z round trip (the separate epilogue kernel cost
    81 us/step + 470 MB of z traffic at the bench shape).
    MIYARN_LT_FWD=0 restores the torch-matmul + epilogue-kernel path."""
    if os.environ.get("MIYARN_LT_FWD", "1") in ("", "0"):
        return False
    return (x.is_cuda and HAVE_EXT and x.dim() == 2
            and x.dtype == torch.bfloat16
            and weight.dtype == torch.bfloat16
            and bias.dtype == torch.bfloat16
            and x.is_contiguous() and weight.is_contiguous())


def _linear_bias_relu_fwd(x: torch.Tensor, weight: torch.Tensor,
                          bias: torch.Tensor) -> torch.Tensor:
    """``relu(x @ weight.T + bias)`` by the first of: the fused ``gemm_bt``
    (opt-in), hipBLASLt with the bias+ReLU epilogue, matmul + the
    ``bias_relu_fwd`` kernel."""
    if _custom_fwd_ok(x, weight, bias):
        return _C.gemm_bt(x, weight, bias, True)
    if _lt_fwd_ok(x, weight, bias):
        return _C.lt_linear(x, weight, bias.contiguous(), True)
    return bias_relu_fwd(x.matmul(weight.t()), bias)


def _linear_wgrad(dz: torch.Tensor, x: torch.Tensor,
                  weight: torch.Tensor) -> torch.Tensor:
    """``dz.T @ x`` in ``weight``'s dtype: the custom split-K kernel where
    :func:`_custom_wgrad_kernel` picks one (split-K partial sum + cast
    fused into one reduce kernel), else the library."""
    kernel = _custom_wgrad_kernel(dz, x)
    if kernel is None:
        return dz.t().matmul(x)
    regstage = True if os.environ.get("MIYARN_WGRAD") == "regstage" else None
    dw = kernel(dz, x, 0, weight.dtype == torch.bfloat16, regstage)
    return dw if dw.dtype == weight.dtype else dw.to(weight.dtype)


class LinearBiasReLU(torch.autograd.Function):
    """y = relu(x @ w.T + bias) with a fully-controlled backward:
    fused dx+dbias kernel, dgrad via hipBLASLt, wgrad via the custom
    split-K MFMA kernel on shapes where it wins."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        y = _linear_bias_relu_fwd(x, weight, bias)
        ctx.save_for_backward(x, weight, y)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, y = ctx.saved_tensors
        dy = dy.contiguous()
        if dy.is_cuda and HAVE_EXT and y.size(-1) % 4 == 0 \
                and y.size(-1) <= 8192:
            dz, dbias = _C.bias_relu_bwd_db(
                dy, y.contiguous(), dy.dtype == torch.bfloat16)
            if dbias.dtype != dy.dtype:
                dbias = dbias.to(dy.dtype)
        else:
            dz = bias_relu_bwd(dy, y)
            dbias = dz.sum(dim=tuple(range(dz.dim() - 1)))
        dx = dz.matmul(weight)
        return dx, _linear_wgrad(dz, x, weight), dbias


def linear_bias_relu(x: torch.Tensor, weight: torch.Tensor,
                     bias: torch.Tensor) -> torch.Tensor:
    return LinearBiasReLU.apply(x, weight, bias)


# ---- last hidden layer + single-logit head ---------------------------------

def fused_head_bwd_enabled() -> bool:
    """MIYARN_FUSED_HEAD_BWD=0 restores the separate last layer and head
    (the head's backward materialises its ``[B, width]`` input gradient)."""
    return _env_switch_on("MIYARN_FUSED_HEAD_BWD")


def head_relu_bwd_db(dl: torch.Tensor, w_head: torch.Tensor,
                     y: torch.Tensor):
    """Backward of "ReLU, then single-logit head" with respect to the
    ReLU's input: ``(dz, dbias)`` of
    ``bias_relu_bwd_db(dl[:, None] * w_head[None, :], y)`` — to the bit —
    without the ``[B, width]`` outer product in memory.  ``dl [B]`` is the
    logit gradient, ``w_head [width]`` the head's weight, ``y [B, width]``
    the ReLU's output.  bf16 widths the oct kernel takes run as one kernel;
    everything else forms the product and takes the two-step path."""
    if _on_gpu(dl, w_head, y) and HAVE_EXT and dl.dtype == y.dtype \
            and w_head.dtype == y.dtype and y.dim() == 2 \
            and y.size(1) % 4 == 0 and y.size(1) <= 8192:
        dz, dbias = _C.head_relu_bwd_db(
            dl.contiguous(), w_head.contiguous(), y.contiguous(),
            y.dtype == torch.bfloat16)
        return dz, dbias.to(y.dtype)
    if _on_gpu(dl, w_head, y):
        _require_ext()
    dz = bias_relu_bwd(dl.unsqueeze(1) * w_head.unsqueeze(0), y)
    return dz, dz.sum(dim=0)


def head_relu_bwd_grads(dl: torch.Tensor, w_head: torch.Tensor,
                        y: torch.Tensor):
    """:func:`head_relu_bwd_db` plus the head's own gradients,
    ``(dz, dbias, dw_head, db_head)`` with ``dw_head = dl^T . y`` and
    ``db_head [1] = dl.sum()`` (fp32 sums stored in ``y``'s dtype).  On the
    GPU, bf16 widths the oct kernel takes run as ONE kernel over ``y`` and
    one reduce for all three vectors; ``dz`` and ``dbias`` are
    :func:`head_relu_bwd_db`'s to the bit.  Other GPU shapes compose
    :func:`col_reduce_dot_sum` and :func:`head_relu_bwd_db`; the CPU runs
    the reference pieces."""
    if _on_gpu(dl, w_head, y) and HAVE_EXT and dl.dtype == y.dtype \
            and w_head.dtype == y.dtype and y.dim() == 2 \
            and y.size(1) % 4 == 0 and y.size(1) <= 8192 \
            and y.dtype in (torch.float32, torch.bfloat16):
        dz, dbias, dw_head, db_head = _C.head_relu_bwd_grads(
            dl.contiguous(), w_head.contiguous(), y.contiguous(),
            y.dtype == torch.bfloat16)
        return dz, dbias, dw_head, db_head
    dw_head = col_reduce_dot(y, dl).to(w_head.dtype)
    db_head = dl.sum().reshape(1).to(w_head.dtype)
    dz, dbias = head_relu_bwd_db(dl, w_head, y)
    return dz, dbias, dw_head, db_head


class LinearBiasReLUHeadFn(torch.autograd.Function):
    """``relu(x @ w.T + bias) . w_head + b_head``: the last hidden layer
    and the single-logit head as ONE autograd node, so that backward goes
    from the logit gradient straight to the layer's ``dz``
    (:func:`head_relu_bwd_db`) instead of writing and re-reading the head's
    ``[B, width]`` input gradient.  Forward is :class:`LinearBiasReLU`'s
    followed by :class:`ScalarHeadFn`'s, backward computes what the two
    nodes computed, kernel for kernel, except for that product."""

    @staticmethod
    def forward(ctx, x, weight, bias, w_head, b_head):
        y = _linear_bias_relu_fwd(x, weight, bias)
        ctx.save_for_backward(x, weight, y, w_head)
        if _on_gpu(y, w_head) and y.size(1) % 4 == 0 \
                and y.size(1) <= 512 and b_head.numel() == 1:
            _require_ext()
            return _C.row_dot(y.contiguous(), w_head.contiguous(),
                              b_head.reshape(1))
        return y @ w_head + b_head

    @staticmethod
    def backward(ctx, dl):
        x, weight, y, w_head = ctx.saved_tensors
        dl = dl.contiguous()
        dw_head = db_head = None
        if ctx.needs_input_grad[3] and ctx.needs_input_grad[4] \
                and _on_gpu(dl, y) and fused_head_grads_enabled():
            dz, dbias, dw_head, db_head = head_relu_bwd_grads(dl, w_head, y)
        else:
            if ctx.needs_input_grad[3]:
                dw_head = col_reduce_dot(y, dl).to(w_head.dtype)
            if ctx.needs_input_grad[4]:
                db_head = dl.sum().reshape(1).to(w_head.dtype)
            dz, dbias = head_relu_bwd_db(dl, w_head, y)
        dx = dz.matmul(weight)
        dw = _linear_wgrad(dz, x, weight)
        return dx, dw, dbias, dw_head, db_head


def linear_bias_relu_head(x: torch.Tensor, weight: torch.Tensor,
                          bias: torch.Tensor, w_head: torch.Tensor,
                          b_head: torch.Tensor) -> torch.Tensor:
    return LinearBiasReLUHeadFn.apply(x, weight, bias, w_head, b_head)


# ---- dgrad + ReLU backward + dbias in one kernel; the tower as one node ----

def fused_dgrad_enabled() -> bool:
    """MIYARN_FUSED_DGRAD=0 keeps every hidden layer's dgrad on the library
    GEMM followed by ``bias_relu_bwd_db``, and the deep tower on one
    autograd node per layer.  Read per call."""
    return _env_switch_on("MIYARN_FUSED_DGRAD")


def _dgrad_drelu_kernel_ok(dz_next: torch.Tensor, weight: torch.Tensor,
                           y: torch.Tensor) -> bool:
    """The preconditions of ``_C.dgrad_drelu`` (``gemm_bt``'s)."""
    if not (HAVE_EXT and dz_next.is_cuda and weight.is_cuda and y.is_cuda):
        return False
    if not (dz_next.dtype == weight.dtype == y.dtype == torch.bfloat16):
        return False
    if not (dz_next.dim() == 2 and weight.dim() == 2 and y.dim() == 2):
        return False
    m, k = dz_next.shape
    n = weight.shape[1]
    return (weight.shape[0] == k and tuple(y.shape) == (m, n) and m > 0
            and m % 256 == 0 and k % 16 == 0 and n % 16 == 0)


def dgrad_drelu(dz_next: torch.Tensor, weight: torch.Tensor,
                y: torch.Tensor):
    """``(dz, dbias)`` of the layer below a hidden layer, from that layer's
    ``dz_next [B, K]``, its weight as stored ``[K, N]`` and the lower
    layer's ReLU output ``y [B, N]``::

        dz    = where(y > 0, dz_next @ weight, 0)     rounded to y's dtype
        dbias = dz.sum(0)                             of the rounded values

    bf16 GPU operands with ``B % 256 == 0`` and ``K``, ``N`` multiples of 16
    run as ONE MFMA kernel (``csrc/dgrad_drelu.hip``) whose epilogue applies
    the mask and forms the column sums, so ``dz_next @ weight`` never
    reaches memory.  Everything else composes the library GEMM and
    :func:`bias_relu_bwd_db`'s kernel, or the plain ops on the CPU."""
    if _dgrad_drelu_kernel_ok(dz_next, weight, y):
        dz, dbias = _C.dgrad_drelu(dz_next.contiguous(),
                                   weight.contiguous(), y.contiguous(),
                                   True)
        return dz, dbias
    return _relu_bwd_db(dz_next.matmul(weight), y)


def _relu_bwd_db(dy: torch.Tensor, y: torch.Tensor):
    """``(dz, dbias)`` from a layer's output gradient, exactly as
    :class:`LinearBiasReLU`'s backward computes them."""
    dy = dy.contiguous()
    if dy.is_cuda and HAVE_EXT and y.size(-1) % 4 == 0 \
            and y.size(-1) <= 8192:
        dz, dbias = _C.bias_relu_bwd_db(
            dy, y.contiguous(), dy.dtype == torch.bfloat16)
        if dbias.dtype != dy.dtype:
            dbias = dbias.to(dy.dtype)
        return dz, dbias
    dz = bias_relu_bwd(dy, y)
    return dz, dz.sum(dim=tuple(range(dz.dim() - 1)))


class MLPHeadFn(torch.autograd.Function):
    """The whole deep tower, ``n`` bias+ReLU layers and the single-logit
    head, as ONE autograd node.  The ReLU mask of layer ``l`` needs
    ``y_l``, which per-layer nodes hand to layer ``l``'s backward; with one
    node, layer ``l+1``'s dgrad can apply it in its own epilogue
    (:func:`dgrad_drelu`).  Forward runs the per-layer nodes' kernels and
    saves the tensors they save; backward computes what they compute,
    kernel for kernel, except on the layers :func:`_fused_dgrad_shape_routed`
    sends to the fused kernel.

    ``apply(x, w_head, b_head, *weights, *biases)``."""

    @staticmethod
    def forward(ctx, x, w_head, b_head, *wb):
        n = len(wb) // 2
        weights, biases = wb[:n], wb[n:]
        ys = []
        h = x
        for w, b in zip(weights, biases):
            h = _linear_bias_relu_fwd(h, w, b)
            ys.append(h)
        ctx.n_layers = n
        ctx.save_for_backward(x, w_head, *weights, *ys)
        if _on_gpu(h, w_head) and h.size(1) % 4 == 0 \
                and h.size(1) <= 512 and b_head.numel() == 1:
            _require_ext()
            return _C.row_dot(h.contiguous(), w_head.contiguous(),
                              b_head.reshape(1))
        return h @ w_head + b_head

    @staticmethod
    def backward(ctx, dl):
        n = ctx.n_layers
        saved = ctx.saved_tensors
        x, w_head = saved[0], saved[1]
        weights, ys = saved[2:2 + n], saved[2 + n:]
        dl = dl.contiguous()
        dw_head = db_head = None
        if ctx.needs_input_grad[1] and ctx.needs_input_grad[2] \
                and _on_gpu(dl, ys[-1]) and fused_head_grads_enabled():
            dz, dbias, dw_head, db_head = head_relu_bwd_grads(
                dl, w_head, ys[-1])
        else:
            if ctx.needs_input_grad[1]:
                dw_head = col_reduce_dot(ys[-1], dl).to(w_head.dtype)
            if ctx.needs_input_grad[2]:
                db_head = dl.sum().reshape(1).to(w_head.dtype)
            dz, dbias = head_relu_bwd_db(dl, w_head, ys[-1])
        dws = [None] * n
        dbs = [None] * n
        fused = fused_dgrad_enabled()
        for l in range(n - 1, 0, -1):
            w, y_below = weights[l], ys[l - 1]
            dws[l] = _linear_wgrad(dz, y_below, w)
            dbs[l] = dbias
            if fused and _fused_dgrad_shape_routed(*w.shape) \
                    and _dgrad_drelu_kernel_ok(dz, w, y_below):
                dz, dbias = dgrad_drelu(dz, w, y_below)
            else:
                dz, dbias = _relu_bwd_db(dz.matmul(w), y_below)
        dx = dz.matmul(weights[0]) if ctx.needs_input_grad[0] else None
        dws[0] = _linear_wgrad(dz, x, weights[0])
        dbs[0] = dbias
        return (dx, dw_head, db_head, *dws, *dbs)


def mlp_bias_relu_head(x: torch.Tensor, weights, biases,
                       w_head: torch.Tensor,
                       b_head: torch.Tensor) -> torch.Tensor:
    """``head(relu(... relu(x @ W_0.T + b_0) ...))`` for a single-logit
    head, as one autograd node (:class:`MLPHeadFn`)."""
    return MLPHeadFn.apply(x, w_head, b_head, *weights, *biases)


def mlp_head_routed(x: torch.Tensor, weights) -> bool:
    """True when :class:`MLPHeadFn` would send at least one hidden layer's
    dgrad of this tower to the fused kernel: the batch is a multiple of
    256, the switch is on and some layer above the first has a routed
    shape."""
    if not (fused_dgrad_enabled() and x.dim() == 2 and x.size(0) > 0
            and x.size(0) % 256 == 0):
        return False
    return any(_fused_dgrad_shape_routed(*w.shape) and w.shape[0] % 16 == 0
               and w.shape[1] % 16 == 0 for w in weights[1:])


# ---- streaming binary-classification eval state ----------------------------

EVAL_BUCKETS = 4096  # score histogram bins, uniform in logit space [-16, 16)
EVAL_SLOTS = 256     # the kernel's maximum grid: one fp64 sums slot per block


class BinaryEvalState:
    """Device state of the streaming binary eval metrics, all zero at start:

    * ``hist`` int64 ``[2, EVAL_BUCKETS]``: histogram of the logits in
      buckets of width 1/128 over ``[-16, 16)`` (both ends clamp), row 0 the
      negatives, row 1 the positives;
    * ``counts`` int64 ``[4]``: ``(n_valid, n_nan, tp, fp)``;
    * ``sums`` float64 ``[EVAL_SLOTS, 2]``: per grid slot
      ``(sum of loss, sum of sigmoid)``.

    Adding two states elementwise is the state of the two streams
    together."""

    def __init__(self, device=None):
        self.hist = torch.zeros(2, EVAL_BUCKETS, dtype=torch.int64,
                                device=device)
        self.counts = torch.zeros(4, dtype=torch.int64, device=device)
        self.sums = torch.zeros(EVAL_SLOTS, 2, dtype=torch.float64,
                                device=device)

    def tensors(self) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        return self.hist, self.counts, self.sums

    def zero_(self) -> "BinaryEvalState":
        for t in self.tensors():
            t.zero_()
        return self


def _binary_eval_update_ref(z: torch.Tensor, y: torch.Tensor,
                            state: BinaryEvalState) -> None:
    """The spec of ``csrc/eval_metrics.hip`` in torch, every per-example
    step in fp32; the sums go to slot 0."""
    nan = torch.isnan(z) | torch.isnan(y)
    n_nan = int(nan.sum())
    z, y = z[~nan], y[~nan]
    pos = y >= 0.5
    hot = z > 0
    # one rounding with or without FMA contraction (both constants are
    # powers of two), so the kernel's bucket is this one to the bit
    t = (z + 16.0) * 128.0
    k = torch.floor(t).clamp_(0.0, EVAL_BUCKETS - 1.0).to(torch.int64)
    state.hist[0] += torch.bincount(k[~pos], minlength=EVAL_BUCKETS)
    state.hist[1] += torch.bincount(k[pos], minlength=EVAL_BUCKETS)
    state.counts += torch.tensor(
        [z.numel(), n_nan, int((pos & hot).sum()), int((~pos & hot).sum())],
        dtype=torch.int64)
    loss = z.clamp_min(0.0) - z * y + torch.log1p(torch.exp(-z.abs()))
    sig = 1.0 / (1.0 + torch.exp(-z))
    state.sums[0, 0] += loss.double().sum()
    state.sums[0, 1] += sig.double().sum()


def binary_eval_update(logits: torch.Tensor, labels: torch.Tensor,
                       state: BinaryEvalState) -> None:
    """Fold a batch of binary-classifier ``logits`` and 0/1 ``labels`` (any
    shapes with equal element counts) into ``state``.  Per example, in
    fp32 (bf16 logits widen exactly; other dtypes are cast)::

        z or y NaN    -> n_nan += 1, nothing else
        pos            = y >= 0.5
        t              = (z + 16) * 128
        k              = 0 if t < 0, 4095 if t >= 4096, else floor(t)
        hist[pos][k]  += 1;  n_valid += 1
        tp += pos and z > 0;  fp += not pos and z > 0
        sums += (max(z,0) - z*y + log1p(exp(-|z|)),  1 / (1 + exp(-z)))

    GPU: one HIP kernel (``csrc/eval_metrics.hip``), no host sync, and the
    same batches in the same order give the same state bit for bit.  CPU:
    the torch reference of the same arithmetic; ``hist`` and ``counts``
    agree with the kernel exactly."""
    z = logits.reshape(-1)
    y = labels.reshape(-1)
    if z.numel() != y.numel():
        raise ValueError(f"{z.numel()} logits but {y.numel()} labels")
    if y.dtype != torch.float32:
        y = y.float()
    if z.numel() == 0:
        return
    if _on_gpu(z, y, *state.tensors()):
        _require_ext()
        if z.dtype not in (torch.float32, torch.bfloat16):
            z = z.float()
        _C.binary_eval_update(z.contiguous(), y.contiguous(),
                              *state.tensors())
        return
    _binary_eval_update_ref(z.float(), y, state)
