"""Criteo wide-and-deep model, MI355X-first.

The reference's target workload family (CTR models trained through the
Keras/Estimator paths; SURVEY §5 "target workloads are CTR/tabular").
Design decisions for MI355X:

* All 26 categorical tables are fused into ONE [total_rows, D] fp32 buffer;
  Python pre-adds per-feature row offsets so the gather/scatter kernels see
  flat ids (:mod:`tf_yarn_amd.ops` ``emb_fwd`` / ``emb_bwd_sgd``).
* The embedding gradient never materializes as a dense table: backward
  stashes (ids, grad_rows); at step time the rows are allgathered across
  data-parallel ranks (equal batch sizes => equal counts, so
  ``all_gather_into_tensor`` over RCCL) and applied with the fused
  atomic scatter+SGD kernel scaled by 1/world.  This replaces the dense
  allreduce that would move the whole table every step.
* Dense compute runs bf16 (``emb_fwd`` fuses the fp32->bf16 cast into the
  gather); dense params keep fp32 master weights.
* The MLP epilogue uses the fused bias+ReLU kernel.
"""

from __future__ import annotations

import logging
import math
from typing import List, NamedTuple, Optional, Tuple

import torch
import torch.distributed as dist
from torch import nn

from tf_yarn_amd import ops

logger = logging.getLogger(__name__)

# Criteo display-advertising schema: 13 integer (dense) + 26 categorical.
CRITEO_DENSE = 13
CRITEO_SPARSE = 26
# Per-feature hash sizes for the synthetic Criteo-1TB-shaped benchmark
# (hashed to 1M rows max per feature, a common Criteo preprocessing).
DEFAULT_TABLE_SIZES = [1_000_000] * CRITEO_SPARSE


# the rules every table accepts, the dim-1 wide table included
SPARSE_OPTIMIZERS = ("sgd", "adagrad", "ftrl")
# tables with dim > 1 also take the rule with one state value per row
DEEP_SPARSE_OPTIMIZERS = SPARSE_OPTIMIZERS + ("rowwise_adagrad",)
# the rules with a per-table step count, accepted for any table, dim 1
# included; kept apart from the two tuples above, which name the rules from
# before lazy Adam
ADAM_SPARSE_OPTIMIZERS = ("lazy_adam",)


def _check_sparse_rule(name: str, value: str, dim: int = 1) -> str:
    """``dim``: the row width of the table the rule is for."""
    if value == "rowwise_adagrad" and dim <= 1:
        raise ValueError(
            f"{name}={value!r}: a dim-1 table's row-wise rule is "
            f"\"adagrad\" (one state value per row already); pick one of "
            f"{SPARSE_OPTIMIZERS + ADAM_SPARSE_OPTIMIZERS}")
    allowed = (DEEP_SPARSE_OPTIMIZERS if dim > 1 else SPARSE_OPTIMIZERS) \
        + ADAM_SPARSE_OPTIMIZERS
    if value not in allowed:
        raise ValueError(
            f"{name} must be one of {allowed}, got {value!r}")
    return value


class _State(NamedTuple):
    """One persistent state buffer of a stateful sparse rule."""
    name: str  # under the table's prefix ("" or "wide_")
    from_init: bool = True  # starts at sparse_initial_accumulator, else at 0
    per_row: bool = False  # shape [rows] instead of the table's


# stateful rule -> its state buffers, in the order the ops take them.  A new
# rule is one entry here.
_RULE_STATES = {
    "adagrad": (_State("state_sum"),),
    "rowwise_adagrad": (_State("state_sum_row", per_row=True),),
    "ftrl": (_State("ftrl_accum"), _State("ftrl_linear", from_init=False)),
    "lazy_adam": (_State("adam_exp_avg", from_init=False),
                  _State("adam_exp_avg_sq", from_init=False)),
}

# the persistent int64 scalar a lazy-Adam table's step count is saved in
_ADAM_STEP = "adam_step"


def _adam_steps_to_buffers(module, prefix, keep_vars) -> None:
    """``state_dict`` pre-hook: write the step counts (Python ints, the
    authority) into their buffers.  A fill, so nothing waits for the
    device."""
    for p, t in module._adam_steps.items():
        getattr(module, p + _ADAM_STEP).fill_(t)


def _adam_steps_before_load(module, state_dict, prefix, *unused) -> None:
    """``load_state_dict`` pre-hook: bring the buffers up to date first, so
    a state dict WITHOUT a step key (``strict=False``) reads back the count
    the module already has, not the one of its last ``state_dict()``."""
    _adam_steps_to_buffers(module, prefix, False)


def _adam_steps_from_buffers(module, incompatible_keys) -> None:
    """``load_state_dict`` post-hook: the one place a step count is read
    back from the device (one ``.item()`` per lazy-Adam table per load)."""
    for p in module._adam_steps:
        module._adam_steps[p] = int(getattr(module, p + _ADAM_STEP).item())


def _default_wide_rule(sparse_optimizer: str) -> str:
    """The wide table's rule when none is given: the deep table's, and
    "adagrad" under a row-wise deep table (the same rule at dim 1)."""
    return ("adagrad" if sparse_optimizer == "rowwise_adagrad"
            else sparse_optimizer)


class SparseOptimizerMixin:
    """Per-table sparse-optimizer choice for the embedding modules.

    The sparse optimizer is chosen ON THE MODEL (``sparse_optimizer=``,
    and ``wide_sparse_optimizer=`` where a module also owns the wide
    table), never inferred from the dense optimizer;
    ``apply_sparse_updates(lr)`` keeps its signature and branches on the
    rule.  ``"sgd"`` (default) adds no attribute that shows in
    ``state_dict``, no memory and no kernel.  A stateful rule adds, per
    table that uses it (``<p>`` is ``""`` or ``"wide_"``):

    * ``"adagrad"``: ``<p>state_sum``; ``"ftrl"``: ``<p>ftrl_accum`` and
      ``<p>ftrl_linear`` — persistent fp32 buffers shaped like the table
      (checkpoints carry them).  ``state_sum`` and ``ftrl_accum`` start at
      ``sparse_initial_accumulator``, ``ftrl_linear`` at 0.  A table owns
      state for its own rule only;
    * ``"rowwise_adagrad"`` (tables with ``dim > 1`` only): ``state_sum_row``,
      ONE persistent fp32 value per row (shape ``[rows]``, filled with
      ``sparse_initial_accumulator``) and no ``state_sum``: ``rows`` floats
      of state instead of ``rows x dim``;
    * ``"lazy_adam"`` (any table): ``<p>adam_exp_avg`` and
      ``<p>adam_exp_avg_sq``, persistent fp32 buffers shaped like the table
      that start at 0 whatever ``sparse_initial_accumulator`` is, and the
      table's step count.  The count is a Python int on the module (no
      apply ever waits for the device to learn it) that advances once per
      applied update of that table; checkpoints carry it as the persistent
      int64 scalar buffer ``<p>adam_step``, which is refreshed from the int
      whenever ``state_dict()`` is taken and read back (one ``.item()``)
      when a state dict is loaded.  Between those two moments the buffer
      may be stale: read ``adam_step_count(<p>)``.  ``sparse_betas`` are
      its betas; ``sparse_eps`` is shared with the Adagrad rules, whose
      default (1e-10) it keeps: pass ``sparse_eps=1e-8`` for Adam's usual;
    * a non-persistent accumulator + int32 row stamp, allocated on the
      first apply (:class:`tf_yarn_amd.ops.SparseWorkspace`, shared by
      the pair whatever their rules).

    All of them are flagged ``_miyarn_sharded`` in every mode so
    ``BucketedDataParallel`` never re-broadcasts a table-sized buffer per
    forward; replicated tables stay consistent because every rank applies
    the same allgathered updates."""

    def _init_sparse_optimizer(self, sparse_eps: float,
                               sparse_initial_accumulator: float,
                               tables: dict, sparse_l1: float = 0.0,
                               sparse_l2: float = 0.0,
                               wide_sparse_lr: Optional[float] = None,
                               sparse_betas: Tuple[float, float] = (0.9,
                                                                    0.999)
                               ) -> None:
        """``tables``: state-name prefix -> (table parameter, rule), deep
        table first; the first stateful entry owns the row stamp."""
        for prefix, (table, rule) in tables.items():
            _check_sparse_rule(f"{prefix}sparse_optimizer", rule,
                               table.shape[1])
        if not (sparse_l1 >= 0 and sparse_l2 >= 0):
            raise ValueError("sparse_l1 and sparse_l2 must be >= 0, got "
                             f"{sparse_l1!r}, {sparse_l2!r}")
        if wide_sparse_lr is not None and not wide_sparse_lr > 0:
            raise ValueError(
                f"wide_sparse_lr must be > 0, got {wide_sparse_lr!r}")
        beta1, beta2 = (float(b) for b in sparse_betas)
        if not (0 <= beta1 < 1 and 0 <= beta2 < 1):
            raise ValueError("sparse_betas must both be in [0, 1), got "
                             f"{sparse_betas!r}")
        self.sparse_betas = (beta1, beta2)
        self.sparse_eps = float(sparse_eps)
        self.sparse_l1 = float(sparse_l1)
        self.sparse_l2 = float(sparse_l2)
        self.wide_sparse_lr = (None if wide_sparse_lr is None
                               else float(wide_sparse_lr))
        self._sparse_buffer_names: List[str] = []
        self._sparse_ws: Optional[ops.SparseWorkspace] = None
        init = float(sparse_initial_accumulator)
        n_stateful = 0
        for prefix, (table, rule) in tables.items():
            if rule == "sgd":
                continue
            names = [prefix + st.name for st in _RULE_STATES[rule]]
            for st in _RULE_STATES[rule]:
                like = table.detach()[:, 0] if st.per_row else table.detach()
                self.register_buffer(
                    prefix + st.name,
                    torch.full(like.shape, init if st.from_init else 0.0,
                               dtype=like.dtype, device=like.device),
                    persistent=True)
            if rule in ADAM_SPARSE_OPTIMIZERS:
                if not hasattr(self, "_adam_steps"):
                    self._adam_steps = {}  # state prefix -> updates applied
                    self.register_state_dict_pre_hook(_adam_steps_to_buffers)
                    self.register_load_state_dict_pre_hook(
                        _adam_steps_before_load)
                    self.register_load_state_dict_post_hook(
                        _adam_steps_from_buffers)
                self._adam_steps[prefix] = 0
                self.register_buffer(
                    prefix + _ADAM_STEP,
                    torch.zeros((), dtype=torch.int64, device=table.device),
                    persistent=True)
                names.append(prefix + _ADAM_STEP)
            acc = ("_adagrad_acc" if n_stateful == 0
                   else f"_adagrad_acc{n_stateful}")
            self.register_buffer(acc, None, persistent=False)
            self._sparse_buffer_names += names + [acc]
            n_stateful += 1
        if n_stateful == 0:
            return
        self.register_buffer("_adagrad_stamp", None, persistent=False)
        self._sparse_buffer_names.append("_adagrad_stamp")
        self._flag_sparse_buffers()

    def _sparse_side(self, rule: str, prefix: str, table: torch.Tensor,
                     grad: torch.Tensor, lr: float) -> "ops.SparseSide":
        """A table's side of a stateful update (``rule`` is not "sgd") with
        this module's state buffers ``<prefix>...`` and scalars.  Every
        applied update of a table builds exactly one side, so this is where
        a lazy-Adam table's step count advances."""
        adam = {}
        if rule in ADAM_SPARSE_OPTIMIZERS:
            self._adam_steps[prefix] += 1
            adam = dict(beta1=self.sparse_betas[0],
                        beta2=self.sparse_betas[1],
                        step=self._adam_steps[prefix])
        return ops.SparseSide(
            rule, table,
            tuple(getattr(self, prefix + st.name)
                  for st in _RULE_STATES[rule]),
            grad, lr, self.sparse_eps, self.sparse_l1, self.sparse_l2, **adam)

    def adam_step_count(self, prefix: str = "") -> int:
        """Updates applied so far to the lazy-Adam table whose state lives
        under ``prefix`` (``""`` or ``"wide_"``)."""
        return self._adam_steps[prefix]

    def _sparse_apply_one(self, rule: str, prefix: str,
                          table: torch.Tensor, ids: torch.Tensor,
                          grad: torch.Tensor, lr: float, scale: float,
                          workspace, wide: bool) -> None:
        """One single-table stateful update."""
        side = self._sparse_side(rule, prefix, table, grad, lr)
        ops.emb_bwd_sparse(ids, **{"wide" if wide else "deep": side},
                           scale=scale, workspace=workspace)

    def _flag_sparse_buffers(self) -> None:
        for name in getattr(self, "_sparse_buffer_names", ()):
            buf = getattr(self, name)
            if buf is not None:
                buf._miyarn_sharded = True

    def _apply(self, fn, *args, **kwargs):
        # .to()/.cuda() replace buffer tensors: carry the flag over
        super()._apply(fn, *args, **kwargs)
        self._flag_sparse_buffers()
        return self

    def __getstate__(self):
        # whole-module pickles (Keras ``save``) and deepcopies leave the
        # scratch behind: it is all-zero / restartable between applies
        state = self.__dict__.copy()
        if state.get("_sparse_ws") is not None:
            state["_sparse_ws"] = None
            buffers = state["_buffers"] = state["_buffers"].copy()
            for name in self._sparse_buffer_names:
                if name.startswith("_adagrad"):
                    buffers[name] = None
        return state

    def _adagrad_workspace(self, table: torch.Tensor,
                           wide_table: Optional[torch.Tensor] = None
                           ) -> "ops.SparseWorkspace":
        """The module's workspace, bound to its non-persistent buffers
        (allocated on first use, re-bound after a device move)."""
        ws = self._sparse_ws
        if ws is None:
            ws = ops.SparseWorkspace(table, wide_table)
            self._sparse_ws = ws
            self._adagrad_acc = ws.acc
            if wide_table is not None:
                self._adagrad_acc1 = ws.wide_acc
            self._adagrad_stamp = ws.stamp
            self._flag_sparse_buffers()
        elif ws.stamp is not self._adagrad_stamp:
            # .to()/unpickling replaced the buffer tensors but kept their
            # contents (zero acc, stamps of past epochs): re-bind
            ws.acc = self._adagrad_acc
            if wide_table is not None:
                ws.wide_acc = self._adagrad_acc1
            ws.stamp = self._adagrad_stamp
        return ws


def _check_combiner(combiner: str) -> str:
    if combiner not in ops.COMBINERS:
        raise ValueError(
            f"combiner must be one of {ops.COMBINERS}, got {combiner!r}")
    return combiner


class BagUpdate(NamedTuple):
    """A sink entry that came from bags (``forward(..., bag_offsets=...)``):
    ``(flat_ids [nnz], grad_rows [nnz, dim])`` like every other entry, but
    ``nnz`` differs from rank to rank, so its data-parallel gather is the
    padded one of :func:`_ragged_all_gather`."""
    flat_ids: torch.Tensor
    grad_rows: torch.Tensor


def _ragged_all_gather(flat_ids: torch.Tensor, rows: torch.Tensor,
                       world: int, process_group):
    """Gather update lists whose length differs by rank.
    ``all_gather_into_tensor`` needs equal counts, so the per-rank counts
    are gathered first (one small collective and one ``.tolist()``, a host
    sync, per table and step), then ids and rows are zero-padded to the
    maximum and gathered asynchronously.  Returns ``(all_ids, all_rows,
    works, counts)``; :func:`_valid_prefixes` drops the padding again, so
    it never reaches an update op."""
    n = flat_ids.numel()
    count = torch.tensor([n], dtype=torch.int64, device=flat_ids.device)
    all_counts = torch.empty(world, dtype=torch.int64,
                             device=flat_ids.device)
    dist.all_gather_into_tensor(all_counts, count, group=process_group)
    counts = all_counts.tolist()
    m = max(counts)
    all_ids = torch.empty(m * world, dtype=flat_ids.dtype,
                          device=flat_ids.device)
    all_rows = torch.empty((m * world,) + tuple(rows.shape[1:]),
                           dtype=rows.dtype, device=rows.device)
    if m == 0:
        return all_ids, all_rows, [], counts
    ids_p = flat_ids.new_zeros(m)
    ids_p[:n] = flat_ids
    rows_p = rows.new_zeros((m,) + tuple(rows.shape[1:]))
    rows_p[:n] = rows
    works = [
        dist.all_gather_into_tensor(all_ids, ids_p, group=process_group,
                                    async_op=True),
        dist.all_gather_into_tensor(all_rows, rows_p, group=process_group,
                                    async_op=True),
    ]
    return all_ids, all_rows, works, counts


def _valid_prefixes(all_ids: torch.Tensor, all_rows: torch.Tensor,
                    counts: Optional[List[int]]):
    """Each rank's valid prefix of a padded gather, concatenated (the
    gather itself when ``counts`` is None: an equal-count entry)."""
    if counts is None:
        return all_ids, all_rows
    m = all_ids.numel() // len(counts)
    if all(c == m for c in counts):
        return all_ids, all_rows
    return (torch.cat([all_ids[r * m:r * m + c]
                       for r, c in enumerate(counts)]),
            torch.cat([all_rows[r * m:r * m + c]
                       for r, c in enumerate(counts)]))


class _FusedLookup(torch.autograd.Function):
    """Gather via the HIP kernel; backward stashes sparse (ids, grad)."""

    @staticmethod
    def forward(ctx, table, flat_ids, out_bf16, sink):
        out = ops.emb_fwd(table, flat_ids, out_bf16)
        ctx.sink = sink
        ctx.save_for_backward(flat_ids)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        (flat_ids,) = ctx.saved_tensors
        ctx.sink.append((flat_ids, grad_out.contiguous()))
        return None, None, None, None


class SparseEmbedding(SparseOptimizerMixin, nn.Module):
    """Fused multi-table embedding with sparse-allgather DP sync.

    ``forward(ids [B, F])`` -> ``[B, F*dim]``.  Multi-hot features:
    ``forward(ids [nnz], bag_offsets [B*F + 1], weights=None)`` pools bag
    ``(b, f)`` with ``combiner`` ("sum", "mean" or "sqrtn";
    :func:`tf_yarn_amd.ops.emb_bag_fwd` has the definition) into the same
    ``[B, F*dim]``; its backward puts ``(flat_ids [nnz], grad_rows [nnz,
    dim])`` into the sink, which every sparse rule consumes unchanged.
    After ``loss.backward()`` call :meth:`apply_sparse_updates` (the
    training loop or the framework optimizer wrapper does this).
    ``sparse_optimizer="adagrad"`` replaces the scatter+SGD update with
    sparse Adagrad (state in the ``state_sum`` buffer), ``"ftrl"`` with
    sparse FTRL-proximal (``ftrl_accum`` / ``ftrl_linear``, regularised
    by ``sparse_l1`` / ``sparse_l2``), ``"rowwise_adagrad"`` (``dim > 1``)
    with row-wise sparse Adagrad, whose whole state is one fp32 value per
    row (``state_sum_row``), ``"lazy_adam"`` with lazy Adam
    (``adam_exp_avg`` / ``adam_exp_avg_sq`` / ``adam_step``, betas from
    ``sparse_betas``).
    """

    def __init__(self, table_sizes: List[int], dim: int,
                 out_bf16: bool = False, init_std: Optional[float] = None,
                 sparse_optimizer: str = "sgd", sparse_eps: float = 1e-10,
                 sparse_initial_accumulator: float = 0.0,
                 sparse_l1: float = 0.0, sparse_l2: float = 0.0,
                 sparse_betas: Tuple[float, float] = (0.9, 0.999),
                 combiner: str = "sum"):
        super().__init__()
        self.table_sizes = list(table_sizes)
        self.dim = dim
        self.combiner = _check_combiner(combiner)
        self.out_bf16 = out_bf16
        total = sum(table_sizes)
        offsets = torch.tensor(
            [0] + list(torch.cumsum(torch.tensor(table_sizes), 0)[:-1]),
            dtype=torch.int64)
        self.register_buffer("offsets", offsets, persistent=True)
        std = init_std if init_std is not None else 1.0 / math.sqrt(dim)
        weight = torch.randn(total, dim) * std
        self.weight = nn.Parameter(weight)
        self.weight._miyarn_sparse = True  # dense reducer must skip it
        self.sparse_optimizer = _check_sparse_rule("sparse_optimizer",
                                                   sparse_optimizer, dim)
        self._init_sparse_optimizer(
            sparse_eps, sparse_initial_accumulator,
            {"": (self.weight, sparse_optimizer)},
            sparse_l1=sparse_l1, sparse_l2=sparse_l2,
            sparse_betas=sparse_betas)
        self._sink: List[Tuple[torch.Tensor, torch.Tensor]] = []

    def forward(self, ids: torch.Tensor,
                bag_offsets: Optional[torch.Tensor] = None,
                weights: Optional[torch.Tensor] = None) -> torch.Tensor:
        if bag_offsets is not None:
            return ops.EmbeddingBagFn.apply(
                self.weight, ids, bag_offsets, len(self.table_sizes),
                self.offsets, weights, self.combiner, self.out_bf16,
                self._sink, None, 0, BagUpdate._make)
        b, f = ids.shape
        assert f == len(self.table_sizes), "feature count mismatch"
        flat = (ids + self.offsets.unsqueeze(0)).reshape(-1)
        out = _FusedLookup.apply(self.weight, flat, self.out_bf16,
                                 self._sink)
        return out.reshape(b, f * self.dim)

    def pending_grads(self) -> List[Tuple[torch.Tensor, torch.Tensor]]:
        return self._sink

    @torch.no_grad()
    def start_sparse_sync(self, process_group=None) -> None:
        """Launch the cross-rank allgather of (ids, grad rows)
        asynchronously (overlaps with the dense optimizer step)."""
        world = (dist.get_world_size(process_group)
                 if dist.is_available() and dist.is_initialized() else 1)
        self._pending_world = world
        self._gathered: List[tuple] = []
        for entry in self._sink:
            flat_ids, grad = entry
            grad2d = grad.reshape(flat_ids.numel(), self.dim)
            if world > 1 and isinstance(entry, BagUpdate):
                # nnz differs by rank: counts first (a host sync), then
                # the padded gather
                self._gathered.append(_ragged_all_gather(
                    flat_ids, grad2d, world, process_group))
            elif world > 1:
                n = flat_ids.numel()
                all_ids = torch.empty(n * world, dtype=flat_ids.dtype,
                                      device=flat_ids.device)
                all_grads = torch.empty((n * world, self.dim),
                                        dtype=grad2d.dtype,
                                        device=grad2d.device)
                works = [
                    dist.all_gather_into_tensor(all_ids, flat_ids,
                                                group=process_group,
                                                async_op=True),
                    dist.all_gather_into_tensor(all_grads, grad2d,
                                                group=process_group,
                                                async_op=True),
                ]
                self._gathered.append((all_ids, all_grads, works, None))
            else:
                # a bag entry carries its count, the mark that lets an
                # all-empty one be skipped
                self._gathered.append((
                    flat_ids, grad2d, [],
                    [flat_ids.numel()] if isinstance(entry, BagUpdate)
                    else None))
        self._sink.clear()

    @torch.no_grad()
    def finish_sparse_sync(self, lr: float) -> None:
        """Wait for the allgathers and apply the fused scatter+SGD (or
        sparse Adagrad) update scaled by 1/world_size."""
        world = getattr(self, "_pending_world", 1)
        for all_ids, all_grads, works, counts in getattr(self, "_gathered",
                                                         []):
            for w in works:
                w.wait()
            all_ids, all_grads = _valid_prefixes(all_ids, all_grads, counts)
            if counts is not None and all_ids.numel() == 0:
                continue  # every bag on every rank was empty
            if self.sparse_optimizer != "sgd":
                self._sparse_apply_one(
                    self.sparse_optimizer, "", self.weight.data, all_ids,
                    all_grads, lr, 1.0 / world,
                    self._adagrad_workspace(self.weight.data), wide=False)
                continue
            ops.emb_bwd_sgd(self.weight.data, all_ids, all_grads,
                            lr=lr, scale=1.0 / world)
        self._gathered = []

    @torch.no_grad()
    def apply_sparse_updates(self, lr: float,
                             process_group=None) -> None:
        """Allgather sparse grads across DP ranks and apply the fused
        scatter+SGD update, scaled by 1/world_size."""
        if not self._sink:
            return
        self.start_sparse_sync(process_group)
        self.finish_sparse_sync(lr)

    def clear_pending(self) -> None:
        self._sink.clear()
        self._gathered = []


class _GatherSum(torch.autograd.Function):
    """Wide-part fused gather-sum: out[b] = sum_f table[ids[b,f]]."""

    @staticmethod
    def forward(ctx, table, flat_ids, batch, out_bf16, sink):
        out = ops.emb_gather_sum(
            table, flat_ids.reshape(batch, -1), out_bf16)
        ctx.sink = sink
        ctx.save_for_backward(flat_ids)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        (flat_ids,) = ctx.saved_tensors
        ctx.sink.append((flat_ids, grad_out.contiguous()))
        return None, None, None, None, None


class WideScalarEmbedding(SparseOptimizerMixin, nn.Module):
    """Per-id scalar weights with fused gather-sum forward and
    scatter-add sparse update (the wide part of wide-and-deep);
    ``sparse_optimizer="adagrad"`` switches the update to sparse
    Adagrad, ``"ftrl"`` to sparse FTRL-proximal (the canonical rule for
    this table; ``sparse_l1 > 0`` leaves exact zeros), ``"lazy_adam"`` to
    lazy Adam.  ``wide_sparse_lr``
    fixes this table's lr whatever ``apply_sparse_updates`` is given.

    Multi-hot features: ``forward(ids [nnz], bag_offsets [B*F + 1],
    weights=None)`` pools every bag at dim 1 with ``combiner``
    (:func:`tf_yarn_amd.ops.emb_bag_fwd`, fp32) and sums the pooled
    ``[B, F]`` over ``f = 0 .. F-1`` into the wide logit; the sink then
    holds ``(flat_ids [nnz], grad [nnz])``, one id per gradient."""

    def __init__(self, table_sizes: List[int], out_bf16: bool = False,
                 init_std: float = 0.01, sparse_optimizer: str = "sgd",
                 sparse_eps: float = 1e-10,
                 sparse_initial_accumulator: float = 0.0,
                 sparse_l1: float = 0.0, sparse_l2: float = 0.0,
                 wide_sparse_lr: Optional[float] = None,
                 sparse_betas: Tuple[float, float] = (0.9, 0.999),
                 combiner: str = "sum"):
        super().__init__()
        self.table_sizes = list(table_sizes)
        self.out_bf16 = out_bf16
        self.combiner = _check_combiner(combiner)
        total = sum(table_sizes)
        offsets = torch.tensor(
            [0] + list(torch.cumsum(torch.tensor(table_sizes), 0)[:-1]),
            dtype=torch.int64)
        self.register_buffer("offsets", offsets, persistent=True)
        self.weight = nn.Parameter(torch.randn(total, 1) * init_std)
        self.weight._miyarn_sparse = True
        self.sparse_optimizer = _check_sparse_rule("sparse_optimizer",
                                                   sparse_optimizer)
        self._init_sparse_optimizer(
            sparse_eps, sparse_initial_accumulator,
            {"": (self.weight, sparse_optimizer)},
            sparse_l1=sparse_l1, sparse_l2=sparse_l2,
            wide_sparse_lr=wide_sparse_lr, sparse_betas=sparse_betas)
        self._sink: List[Tuple[torch.Tensor, torch.Tensor]] = []

    def forward(self, ids: torch.Tensor,
                bag_offsets: Optional[torch.Tensor] = None,
                weights: Optional[torch.Tensor] = None) -> torch.Tensor:
        if bag_offsets is not None:
            # pooled in fp32 and rounded once after the sum over features,
            # as the one-hot gather-sum rounds
            pooled = ops.EmbeddingBagFn.apply(
                self.weight, ids, bag_offsets, len(self.table_sizes),
                self.offsets, weights, self.combiner, False, self._sink,
                None, 0, self._bag_update)
            out = pooled.sum(dim=1)
            return out.to(torch.bfloat16) if self.out_bf16 else out
        b = ids.shape[0]
        flat = (ids + self.offsets.unsqueeze(0)).reshape(-1)
        return _GatherSum.apply(self.weight, flat, b, self.out_bf16,
                                self._sink)

    @staticmethod
    def _bag_update(entry) -> BagUpdate:
        flat_ids, rows = entry
        return BagUpdate(flat_ids, rows.reshape(-1))  # [nnz, 1] -> [nnz]

    def pending_grads(self):
        return self._sink

    @torch.no_grad()
    def start_sparse_sync(self, process_group=None) -> None:
        world = (dist.get_world_size(process_group)
                 if dist.is_available() and dist.is_initialized() else 1)
        self._pending_world = world
        self._gathered = []
        for entry in self._sink:
            flat_ids, grad = entry
            if world > 1 and isinstance(entry, BagUpdate):
                self._gathered.append(_ragged_all_gather(
                    flat_ids, grad.reshape(-1), world, process_group))
            elif world > 1:
                n = flat_ids.numel()
                b = grad.numel()
                all_ids = torch.empty(n * world, dtype=flat_ids.dtype,
                                      device=flat_ids.device)
                all_grads = torch.empty(b * world, dtype=grad.dtype,
                                        device=grad.device)
                works = [
                    dist.all_gather_into_tensor(all_ids, flat_ids,
                                                group=process_group,
                                                async_op=True),
                    dist.all_gather_into_tensor(all_grads,
                                                grad.reshape(-1),
                                                group=process_group,
                                                async_op=True),
                ]
                self._gathered.append((all_ids, all_grads, works, None))
            else:
                self._gathered.append((
                    flat_ids, grad.reshape(-1), [],
                    [flat_ids.numel()] if isinstance(entry, BagUpdate)
                    else None))
        self._sink.clear()

    @torch.no_grad()
    def finish_sparse_sync(self, lr: float) -> None:
        world = getattr(self, "_pending_world", 1)
        if self.wide_sparse_lr is not None:
            lr = self.wide_sparse_lr
        for all_ids, all_grads, works, counts in getattr(self, "_gathered",
                                                         []):
            for w in works:
                w.wait()
            all_ids, all_grads = _valid_prefixes(all_ids, all_grads, counts)
            if counts is not None and all_ids.numel() == 0:
                continue
            if self.sparse_optimizer != "sgd":
                self._sparse_apply_one(
                    self.sparse_optimizer, "", self.weight.data, all_ids,
                    all_grads, lr, 1.0 / world,
                    self._adagrad_workspace(self.weight.data), wide=True)
                continue
            ops.emb_scatter_sum(self.weight.data,
                                all_ids.reshape(all_grads.numel(), -1),
                                all_grads, alpha=-lr / world)
        self._gathered = []

    @torch.no_grad()
    def apply_sparse_updates(self, lr: float, process_group=None) -> None:
        if not self._sink:
            return
        self.start_sparse_sync(process_group)
        self.finish_sparse_sync(lr)

    def clear_pending(self) -> None:
        self._sink.clear()
        self._gathered = []


class _DeepInput(torch.autograd.Function):
    """Build the MLP input [B, dense_pad + F*dim] in ONE buffer: dense
    features go to columns [0:13] (padded to 16 for quad alignment) and the
    embedding gather writes straight into the rest (no concat kernel).
    Backward stashes the embedding slice of the grad as the sparse sink."""

    DENSE_PAD = 16

    @staticmethod
    def forward(ctx, dense, table, flat_ids, dim, out_bf16, sink):
        b = dense.shape[0]
        f = flat_ids.numel() // b
        dtype = torch.bfloat16 if out_bf16 else torch.float32
        out = torch.empty(b, _DeepInput.DENSE_PAD + f * dim,
                          dtype=dtype, device=dense.device)
        out[:, :dense.shape[1]] = dense.to(dtype)
        out[:, dense.shape[1]:_DeepInput.DENSE_PAD] = 0
        ops.emb_fwd_into(table, flat_ids, out, _DeepInput.DENSE_PAD)
        ctx.sink = sink
        ctx.save_for_backward(flat_ids)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        (flat_ids,) = ctx.saved_tensors
        emb_grad = grad_out[:, _DeepInput.DENSE_PAD:].contiguous()
        ctx.sink.append((flat_ids, emb_grad))
        return None, None, None, None, None, None


class ScalarHead(nn.Module):
    """Single-logit head as a GEMV: ``logits[b] = x[b] . w + bias``.

    An nn.Linear(in, 1) makes autograd emit an M=1, K=batch wgrad GEMM
    that hipBLASLt runs terribly (140 us measured for 33 MFLOP); the mv
    form lowers to GEMV/broadcast kernels instead."""

    def __init__(self, in_features: int, dtype=torch.float32):
        super().__init__()
        bound = 1.0 / math.sqrt(in_features)
        self.weight = nn.Parameter(
            (torch.rand(in_features, dtype=torch.float32) * 2 - 1) * bound)
        self.bias = nn.Parameter(torch.zeros(1, dtype=torch.float32))
        if dtype != torch.float32:
            self.weight.data = self.weight.data.to(dtype)
            self.bias.data = self.bias.data.to(dtype)

    def forward(self, x):
        if x.size(-1) % 4 == 0:
            return ops.ScalarHeadFn.apply(x, self.weight, self.bias)
        if x.is_cuda:
            # Ragged width (e.g. the 13 raw dense features): hipBLASLt
            # runs this bias-GEMV at ~9 GB/s (192 us measured at
            # 65536x13); zero-pad to a quad boundary and take the
            # streaming row_dot path instead (~2 us pad + ~5 us dot).
            pad = (-x.size(-1)) % 4
            xp = nn.functional.pad(x, (0, pad))
            wp = nn.functional.pad(self.weight, (0, pad))
            return ops.ScalarHeadFn.apply(xp, wp, self.bias)
        return x @ self.weight + self.bias


class FusedLinearReLU(nn.Module):
    """Linear (library GEMM) + fused bias+ReLU epilogue kernel."""

    def __init__(self, in_features: int, out_features: int,
                 dtype=torch.float32):
        super().__init__()
        self.weight = nn.Parameter(
            torch.empty(out_features, in_features, dtype=dtype))
        self.bias = nn.Parameter(torch.zeros(out_features, dtype=dtype))
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))

    def forward(self, x):
        return ops.linear_bias_relu(x, self.weight, self.bias)


class WideAndDeep(nn.Module):
    """Wide (per-id scalar weights) + deep (embeddings -> MLP) CTR model."""

    def __init__(self,
                 dense_dim: int = CRITEO_DENSE,
                 table_sizes: Optional[List[int]] = None,
                 embedding_dim: int = 16,
                 hidden: Tuple[int, ...] = (1024, 512, 256),
                 compute_dtype: torch.dtype = torch.float32,
                 sharded: bool = False,
                 process_group=None,
                 sparse_optimizer: str = "sgd",
                 sparse_eps: float = 1e-10,
                 sparse_initial_accumulator: float = 0.0,
                 wide_sparse_optimizer: Optional[str] = None,
                 sparse_l1: float = 0.0, sparse_l2: float = 0.0,
                 wide_sparse_lr: Optional[float] = None,
                 sparse_betas: Tuple[float, float] = (0.9, 0.999),
                 combiner: str = "sum"):
        """``sparse_optimizer`` ("sgd", "adagrad", "ftrl", "lazy_adam" or
        "rowwise_adagrad") picks the update rule of the embedding tables;
        it is NOT inferred from the dense optimizer, whose lr is what
        ``apply_sparse_updates(lr)`` receives.  ``wide_sparse_optimizer``
        picks the wide table's rule (None: the same as
        ``sparse_optimizer``), so the textbook wide-and-deep recipe is
        ``sparse_optimizer="adagrad", wide_sparse_optimizer="ftrl",
        sparse_l1=...``.

        ``"rowwise_adagrad"`` keeps one state value per deep ROW
        (``state_sum_row``, ``rows`` floats instead of ``rows x dim``).
        It is a rule for the deep table only: the wide table is dim 1,
        where the same rule is ``"adagrad"``, which is also its default
        under a row-wise deep table; ``wide_sparse_optimizer=
        "rowwise_adagrad"`` raises ``ValueError``.

        ``sparse_l1`` / ``sparse_l2``: FTRL's regularisation strengths
        (L1 > 0 is what makes untrained-away weights exactly 0).
        ``wide_sparse_lr``: when set, the wide table runs at this fixed
        lr instead of the one passed to ``apply_sparse_updates``.
        ``sparse_initial_accumulator`` fills Adagrad's ``state_sum`` and
        FTRL's ``ftrl_accum`` alike; TF's default for both is 0.1.

        ``"lazy_adam"`` (any table; the wide table follows the deep one by
        default) is ``torch.optim.SparseAdam`` / TF ``LazyAdam``: only the
        batch's rows move, with ``sparse_betas`` and one step count per
        table that checkpoints carry (``adam_step``).  Its ``eps`` is
        ``sparse_eps``, whose default 1e-10 is Adagrad's (Adam's usual is
        1e-8), outside the square root; its two states start at 0 and
        ignore ``sparse_initial_accumulator``.

        ``combiner`` ("sum", "mean" or "sqrtn") pools multi-hot features:
        ``forward(dense, ids [nnz], labels, bag_offsets=[B*F + 1],
        sparse_weights=None)`` (replicated tables only; the one-hot call
        ``forward(dense, ids [B, F])`` is unchanged and ignores it)."""
        super().__init__()
        table_sizes = table_sizes or DEFAULT_TABLE_SIZES
        self.combiner = _check_combiner(combiner)
        if wide_sparse_optimizer is None:
            wide_sparse_optimizer = _default_wide_rule(sparse_optimizer)
        sparse_kw = dict(
            sparse_optimizer=sparse_optimizer, sparse_eps=sparse_eps,
            sparse_initial_accumulator=sparse_initial_accumulator,
            sparse_l1=sparse_l1, sparse_l2=sparse_l2,
            sparse_betas=sparse_betas)
        self.sparse_optimizer = sparse_optimizer
        self.wide_sparse_optimizer = wide_sparse_optimizer
        self.compute_dtype = compute_dtype
        self.dense_dim = dense_dim
        bf16 = compute_dtype == torch.bfloat16
        self.sharded = sharded
        if sharded:
            from tf_yarn_amd.models.sharded_embedding import \
                ShardedCriteoEmbeddings
            self.embeddings = ShardedCriteoEmbeddings(
                table_sizes, embedding_dim, out_bf16=bf16,
                process_group=process_group,
                wide_sparse_optimizer=wide_sparse_optimizer,
                wide_sparse_lr=wide_sparse_lr, **sparse_kw)
            self.deep_embedding = None
            self.wide_embedding = None
        else:
            self.embeddings = None
            self.deep_embedding = SparseEmbedding(
                table_sizes, embedding_dim, out_bf16=bf16,
                combiner=combiner, **sparse_kw)
            # Wide: one scalar weight per categorical id
            wide_kw = dict(sparse_kw, sparse_optimizer=wide_sparse_optimizer,
                           wide_sparse_lr=wide_sparse_lr, combiner=combiner)
            self.wide_embedding = WideScalarEmbedding(table_sizes,
                                                      out_bf16=bf16,
                                                      **wide_kw)
        self.wide_dense = ScalarHead(dense_dim, compute_dtype)
        layers: List[nn.Module] = []
        # dense block padded to 16 columns for quad-aligned fused gather
        in_dim = _DeepInput.DENSE_PAD + len(table_sizes) * embedding_dim
        for h in hidden:
            layers.append(FusedLinearReLU(in_dim, h))
            in_dim = h
        self.mlp = nn.Sequential(*layers)
        self.head = ScalarHead(in_dim, compute_dtype)
        if bf16:
            # dense compute in bf16; masters are managed by the optimizer
            self.mlp = self.mlp.to(torch.bfloat16)

    def _deep_tower(self, deep_in: torch.Tensor) -> torch.Tensor:
        """``head(mlp(deep_in))``.  On the GPU in bf16 the last hidden
        layer and the head run as one autograd node whose backward never
        materialises the head's ``[B, width]`` input gradient
        (``ops.LinearBiasReLUHeadFn``; same kernels and bits otherwise).
        MIYARN_FUSED_HEAD_BWD=0 keeps the two modules apart.  At a batch
        that is a multiple of 256, a tower with a hidden layer whose dgrad
        shape is routed to ``ops.dgrad_drelu`` runs as ``ops.MLPHeadFn``."""
        n = len(self.mlp)
        last = self.mlp[n - 1] if n else None
        head = self.head
        if not (isinstance(last, FusedLinearReLU) and deep_in.is_cuda
                and ops.HAVE_EXT and deep_in.dim() == 2
                and deep_in.dtype == torch.bfloat16
                and last.weight.dtype == torch.bfloat16
                and last.bias.dtype == torch.bfloat16
                and head.weight.dtype == torch.bfloat16
                and head.bias.dtype == torch.bfloat16
                and last.weight.shape[0] % 4 == 0
                and ops.fused_head_bwd_enabled()):
            return head(self.mlp(deep_in))
        # The whole tower as one node where a hidden layer's dgrad is
        # routed to the kernel that applies the ReLU mask of the layer
        # below in its epilogue (ops.MLPHeadFn; MIYARN_FUSED_DGRAD=0
        # keeps the per-layer nodes).
        if all(isinstance(m, FusedLinearReLU)
               and m.weight.dtype == torch.bfloat16
               and m.bias.dtype == torch.bfloat16 for m in self.mlp):
            weights = [m.weight for m in self.mlp]
            if ops.mlp_head_routed(deep_in, weights):
                return ops.mlp_bias_relu_head(
                    deep_in, weights, [m.bias for m in self.mlp],
                    head.weight, head.bias)
        h = deep_in
        for i in range(n - 1):
            h = self.mlp[i](h)
        return ops.linear_bias_relu_head(h, last.weight, last.bias,
                                         head.weight, head.bias)

    def forward(self, dense: torch.Tensor, sparse_ids: torch.Tensor,
                labels: Optional[torch.Tensor] = None,
                bag_offsets: Optional[torch.Tensor] = None,
                sparse_weights: Optional[torch.Tensor] = None
                ) -> torch.Tensor:
        """Returns logits [B], or — when ``labels`` is given — the mean
        BCEWithLogits loss with the 3-part logit sum fused into the loss
        kernel (ops.bce_head_loss).

        With ``bag_offsets`` (``[B*F + 1]``) the features are multi-hot:
        ``sparse_ids`` is the flat ``[nnz]`` id array, bag ``b*F + f``
        holds the ids of feature ``f`` of example ``b`` (optionally
        weighted by ``sparse_weights [nnz]``) and is pooled by the model's
        ``combiner``.  The MLP input is built in one buffer: the dense
        columns, zeros up to ``_DeepInput.DENSE_PAD``, and the pooled
        lookup written straight into the slice behind them."""
        dense = dense.to(self.compute_dtype)
        if bag_offsets is not None:
            if self.sharded:
                raise NotImplementedError(
                    "multi-hot input (bag_offsets) with sharded=True: the "
                    "feature-sharded all-to-all of ragged bags is not "
                    "built; use the replicated tables (sharded=False)")
            emb = self.deep_embedding
            deep_in = ops.EmbeddingBagFn.apply(
                emb.weight, sparse_ids, bag_offsets, len(emb.table_sizes),
                emb.offsets, sparse_weights, self.combiner,
                self.compute_dtype == torch.bfloat16, emb._sink, dense,
                _DeepInput.DENSE_PAD, BagUpdate._make)
            deep_out = self._deep_tower(deep_in)
            wide_emb = self.wide_embedding(
                sparse_ids, bag_offsets, sparse_weights).to(deep_out.dtype)
            wd = self.wide_dense(dense)
            if labels is not None:
                return ops.bce_head_loss(deep_out, wide_emb, wd, labels)
            return deep_out + wide_emb + wd
        if sparse_weights is not None:
            raise ValueError("sparse_weights needs bag_offsets")
        if self.sharded:
            b = dense.shape[0]
            emb = self.embeddings
            deep_in = torch.empty(
                b, _DeepInput.DENSE_PAD + emb.F * emb.dim,
                dtype=self.compute_dtype, device=dense.device)
            # the lookup also writes the dense and pad columns (one
            # kernel with the gather on a single GPU)
            deep_in, wide_sum = emb(sparse_ids, deep_in,
                                    _DeepInput.DENSE_PAD, dense=dense)
            deep_out = self._deep_tower(deep_in)
            wide_sum = wide_sum.to(deep_out.dtype)
            wd = self.wide_dense(dense)
            if labels is not None:
                return ops.bce_head_loss(deep_out, wide_sum, wd, labels)
            return deep_out + wide_sum + wd
        emb = self.deep_embedding
        flat = (sparse_ids + emb.offsets.unsqueeze(0)).reshape(-1)
        deep_in = _DeepInput.apply(
            dense, emb.weight, flat, emb.dim,
            self.compute_dtype == torch.bfloat16, emb._sink)
        deep_out = self._deep_tower(deep_in)
        wide_emb = self.wide_embedding(sparse_ids).to(deep_out.dtype)
        wd = self.wide_dense(dense)
        if labels is not None:
            return ops.bce_head_loss(deep_out, wide_emb, wd, labels)
        return deep_out + wide_emb + wd

    def start_sparse_sync(self, process_group=None) -> None:
        """Kick off the replicated-mode allgathers (called right after
        ``loss.backward()`` so communication overlaps with the dense
        optimizer step).  Sharded mode already exchanged grads during
        backward (all-to-all), so there is nothing to start."""
        if self.sharded:
            return
        self.deep_embedding.start_sparse_sync(process_group)
        self.wide_embedding.start_sparse_sync(process_group)

    def finish_sparse_sync(self, lr: float, stream=None) -> None:
        if self.sharded:
            self.embeddings.apply_sparse_updates(lr, stream=stream)
            return
        self.deep_embedding.finish_sparse_sync(lr)
        self.wide_embedding.finish_sparse_sync(lr)

    def apply_sparse_updates(self, lr: float, process_group=None) -> None:
        self.start_sparse_sync(process_group)
        self.finish_sparse_sync(lr)

    def clear_pending(self) -> None:
        if self.sharded:
            self.embeddings.clear_pending()
            return
        self.deep_embedding.clear_pending()
        self.wide_embedding.clear_pending()


class FlatInputWideAndDeep(nn.Module):
    """WideAndDeep behind a single-tensor input — the shape the Keras
    ``fit(x, y)`` / Estimator ``input_fn`` surfaces expect:
    ``x = [dense fp32 columns | categorical id columns]``.  Importable
    (not example-local) so whole-model Keras checkpoints pickle."""

    def __init__(self, dense_dim: int = CRITEO_DENSE,
                 table_sizes: Optional[List[int]] = None,
                 embedding_dim: int = 16,
                 hidden: Tuple[int, ...] = (1024, 512, 256),
                 compute_dtype: torch.dtype = torch.float32,
                 sharded: bool = False, process_group=None,
                 sparse_optimizer: str = "sgd", sparse_eps: float = 1e-10,
                 sparse_initial_accumulator: float = 0.0,
                 wide_sparse_optimizer: Optional[str] = None,
                 sparse_l1: float = 0.0, sparse_l2: float = 0.0,
                 wide_sparse_lr: Optional[float] = None,
                 sparse_betas: Tuple[float, float] = (0.9, 0.999)):
        """The sparse-optimizer arguments are :class:`WideAndDeep`'s."""
        super().__init__()
        self.dense_dim = dense_dim
        init_acc = sparse_initial_accumulator
        self.net = WideAndDeep(dense_dim=dense_dim,
                               sparse_optimizer=sparse_optimizer,
                               sparse_eps=sparse_eps,
                               sparse_initial_accumulator=init_acc,
                               wide_sparse_optimizer=wide_sparse_optimizer,
                               sparse_l1=sparse_l1, sparse_l2=sparse_l2,
                               wide_sparse_lr=wide_sparse_lr,
                               sparse_betas=sparse_betas,
                               table_sizes=table_sizes,
                               embedding_dim=embedding_dim, hidden=hidden,
                               compute_dtype=compute_dtype,
                               sharded=sharded,
                               process_group=process_group)

    def forward(self, x: torch.Tensor,
                labels: Optional[torch.Tensor] = None) -> torch.Tensor:
        dense = x[:, :self.dense_dim]
        ids = x[:, self.dense_dim:].long()
        return self.net(dense, ids, labels=labels)

    def start_sparse_sync(self, process_group=None) -> None:
        self.net.start_sparse_sync(process_group)

    def finish_sparse_sync(self, lr: float, stream=None) -> None:
        self.net.finish_sparse_sync(lr, stream=stream)

    def apply_sparse_updates(self, lr: float, process_group=None) -> None:
        self.net.apply_sparse_updates(lr, process_group)

    def clear_pending(self) -> None:
        self.net.clear_pending()
