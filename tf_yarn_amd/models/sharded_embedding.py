"""Feature-sharded embeddings with all-to-all exchange (model-parallel
embeddings, DLRM-style) — the xGMI-native scaling path.

With replicated tables, data-parallel sparse sync needs an allgather of
every rank's (ids, grad rows): ~54 MB/rank/step at batch 65536, which a
ring allgather moves in ~2.5 ms over 8 GPUs — more than the whole 1-GPU
step.  xGMI is 7 point-to-point links per GPU, so ALL-TO-ALL traffic
rides all links concurrently; sharding the 26 categorical tables across
ranks (rank r owns features f with f % world == r) turns the sparse
exchange into two all-to-alls (~48 MB each way, ~0.2 ms) and makes every
table row owner-updated (no cross-rank gradient dup at all).

Flow per step (world W, local batch B, F features, dim D):
  fwd:  ids[:, feats_of(s)] --all-to-all--> owners gather their shard
        (fused HIP kernel, bf16 out) --all-to-all--> [B, F*D] assembled
        straight into the MLP input buffer; the wide part reuses the SAME
        routed ids, owners compute partial gather-sums, tiny all-to-all
        back.
  bwd:  grad slices --all-to-all--> owners stash (ids, grads); the wide
        grad is a small allgather.
  update: owner-local fused scatter+SGD, scale 1/W (no further comm).

W == 1 degenerates to the local fused path with zero communication.
gloo has no all_to_all: a correctness-equivalent allgather+slice
emulation backs the CPU tests (`_all_to_all_single`).
"""

from __future__ import annotations

import logging
import weakref
from typing import List, Optional, Tuple

import torch
import torch.distributed as dist
from torch import nn

from tf_yarn_amd import ops
from tf_yarn_amd.models.wide_deep import (SparseOptimizerMixin,
                                          _default_wide_rule)
from tf_yarn_amd.utils import commprobe

logger = logging.getLogger(__name__)


def _world_rank(group) -> Tuple[int, int]:
    if dist.is_available() and dist.is_initialized():
        return dist.get_world_size(group), dist.get_rank(group)
    return 1, 0


# Per-group probe cache, weak-keyed on the ProcessGroup object itself so a
# destroyed+gc'd group can never alias a new group's entry (id() reuse).
_ALLTOALL_MODE: "weakref.WeakKeyDictionary" = weakref.WeakKeyDictionary()


# Binned scatter pays only when ids repeat (the LDS-hash dedup divides
# the table RMW traffic by the duplication factor but costs a ~200 us
# permutation).  From the round-2 A/B at the bench shape: atomic 422 us
# flat; binned perm ~200 + applies that scale with unique/n — break-even
# near duplication factor ~2.
# NOTE: the atomic kernel has since dropped to ~177 us on uniform ids and
# ~960 us on Zipf(1.2) ids (row-segment map, docs/Kernels.md), so this
# break-even is stale and sits higher now; it has not been re-measured.
SKEW_THRESHOLD = 2.0


def _binned_mode() -> str:
    """MIYARN_BINNED_SCATTER: '1' force on, '0' force off, unset/'auto'
    = probe the id distribution once and decide (uniform ids keep the
    measured-fastest atomic kernels; power-law CTR traffic flips to the
    dedup path automatically)."""
    import os
    v = os.environ.get("MIYARN_BINNED_SCATTER", "auto")
    if v == "1":
        return "on"
    if v in ("", "0"):
        return "off"
    return "auto"


def negotiated_alltoall_mode(group=None) -> str:
    """The mode the self-check picked for this group: 'native',
    'emulate', 'gloo-emulate', or 'unprobed' (reported in bench.py's
    JSON so a silent fallback is visible in the scale run)."""
    if not (dist.is_available() and dist.is_initialized()):
        return "unprobed"
    if dist.get_backend(group) == "gloo":
        return "gloo-emulate"
    key = (group if group is not None
           else dist.distributed_c10d._get_default_group())
    return _ALLTOALL_MODE.get(key, "unprobed")


def _perm_stream_enabled() -> bool:
    import os
    v = os.environ.get("MIYARN_PERM_STREAM", "1")
    return v != "" and v != "0"


def _alltoall_self_check(group=None) -> str:
    """One-time probe: every rank sends rank*100+dest to dest; verify the
    native all_to_all_single delivers it.  On any mismatch or error the
    group permanently falls back to the allgather emulation (correct on
    every backend) — insurance for the unattended 8-GPU scale run."""
    world = dist.get_world_size(group)
    rank = dist.get_rank(group)
    device = (torch.device("cuda", torch.cuda.current_device())
              if dist.get_backend(group) == "nccl" else "cpu")
    send = torch.tensor([rank * 100 + d for d in range(world)],
                        dtype=torch.int64, device=device)
    recv = torch.zeros(world, dtype=torch.int64, device=device)
    try:
        dist.all_to_all_single(recv, send,
                               output_split_sizes=[1] * world,
                               input_split_sizes=[1] * world, group=group)
        expected = torch.tensor([s * 100 + rank for s in range(world)],
                                dtype=torch.int64, device=device)
        ok = bool(torch.equal(recv, expected))
    except Exception:  # noqa: BLE001
        ok = False
    # every rank must agree on the mode
    flag = torch.tensor([1 if ok else 0], dtype=torch.int64,
                        device=device)
    dist.all_reduce(flag, op=dist.ReduceOp.MIN, group=group)
    mode = "native" if int(flag.item()) == 1 else "emulate"
    if mode == "emulate":
        logger.warning("all_to_all_single self-check failed; using the "
                       "allgather emulation for this group")
    return mode


def _all_to_all_single(output: torch.Tensor, input_: torch.Tensor,
                       out_splits: List[int], in_splits: List[int],
                       group=None) -> None:
    """dist.all_to_all_single with a gloo fallback (allgather + slice) so
    the distributed path is testable on CPU (gloo lacks alltoall), plus a
    one-time native self-check on other backends."""
    backend = dist.get_backend(group)
    if backend != "gloo":
        key = (group if group is not None
               else dist.distributed_c10d._get_default_group())
        mode = _ALLTOALL_MODE.get(key)
        if mode is None:
            mode = _alltoall_self_check(group)
            _ALLTOALL_MODE[key] = mode
        if mode == "native":
            dist.all_to_all_single(output, input_,
                                   output_split_sizes=out_splits,
                                   input_split_sizes=in_splits,
                                   group=group)
            return
    world = dist.get_world_size(group)
    rank = dist.get_rank(group)
    # Emulation: allgather every rank's full input (+ splits), then take
    # the chunk addressed to this rank from each peer.
    my_splits = torch.tensor(in_splits, dtype=torch.int64)
    all_splits = [torch.zeros(world, dtype=torch.int64)
                  for _ in range(world)]
    dist.all_gather(all_splits, my_splits, group=group)
    max_numel = max(int(s.sum()) for s in all_splits)
    padded = torch.zeros(max_numel, dtype=input_.dtype,
                         device=input_.device)
    padded[:input_.numel()] = input_.reshape(-1)
    gathered = [torch.zeros_like(padded) for _ in range(world)]
    dist.all_gather(gathered, padded, group=group)
    offset = 0
    for p in range(world):
        splits_p = all_splits[p].tolist()
        start = sum(splits_p[:rank])
        n = splits_p[rank]
        output.reshape(-1)[offset:offset + n] = \
            gathered[p][start:start + n]
        offset += n


class _ShardedLookup(torch.autograd.Function):
    """Forward/backward all-to-all routing around the owner-local fused
    gather; backward stashes owner-local (ids, grads) in the sink."""

    @staticmethod
    def forward(ctx, deep_table, wide_table, module, ids, deep_out_buf,
                col_offset, dense=None, grad_enabled=False):
        # grad_enabled: the caller's grad mode (autograd has switched it
        # off in here); a permutation is prefetched only for a forward
        # that a backward can follow
        m: "ShardedCriteoEmbeddings" = module
        W, B = m.world, ids.shape[0]
        D = m.dim
        device = ids.device
        ctx.raw_ids = False

        if W == 1 and dense is not None and m._fused_lookup_ok(
                ids, dense, deep_out_buf, col_offset):
            # One kernel from the RAW ids: offset add, deep gather, wide
            # gather-sum and the dense / pad columns.  The fused SGD
            # scatter adds the offsets itself too, so no flat-id array
            # exists on this path; every other consumer of the ids (the
            # binned scatter and its permutation, the stateful rules, a
            # wide lr of its own) keeps the pre-added array.
            ids = ids.contiguous()
            wide_out = ops.emb_lookup_fused(
                deep_table, wide_table, ids, m.full_offsets, dense,
                deep_out_buf, col_offset)
            if m._scatter_takes_raw_ids():
                saved = ids
                ctx.raw_ids = True
            else:
                saved = (ids + m.full_offsets.unsqueeze(0)).reshape(-1)
                m._start_perm_async(saved, grad_enabled)
            ctx.module = m
            ctx.save_for_backward(saved)
            ctx.local_only = True
            ctx.mark_dirty(deep_out_buf)
            return deep_out_buf, wide_out

        if dense is not None:
            deep_out_buf[:, :dense.shape[1]] = dense
            deep_out_buf[:, dense.shape[1]:col_offset] = 0

        if W == 1:
            flat = (ids + m.full_offsets.unsqueeze(0)).reshape(-1)
            ops.emb_fwd_into(deep_table, flat, deep_out_buf, col_offset)
            wide_out = ops.emb_gather_sum(wide_table, flat.reshape(B, -1),
                                          m.out_bf16)
            m._start_perm_async(flat, grad_enabled)
            ctx.module = m
            ctx.save_for_backward(flat)
            ctx.local_only = True
            ctx.mark_dirty(deep_out_buf)
            return deep_out_buf, wide_out

        # ---- route ids to owners ----------------------------------------
        # send chunk for peer s: ids[:, feats_of(s)] row-major [B, F_s]
        ids_send = torch.cat(
            [ids[:, m.feats_of[s]].reshape(-1) for s in range(W)])
        in_splits = [B * len(m.feats_of[s]) for s in range(W)]
        n_own = B * m.f_own
        ids_recv = torch.empty(W * n_own, dtype=torch.int64, device=device)
        with commprobe.span("a2a_ids"):
            _all_to_all_single(ids_recv, ids_send, [n_own] * W, in_splits,
                               m.group)
        # local row offsets: layout [peer][b][j], j = feature slot
        flat_local = ids_recv + m.own_offsets_tiled[:ids_recv.numel()]

        m._start_perm_async(flat_local, grad_enabled)

        # ---- owner-local gathers ----------------------------------------
        vec = ops.emb_fwd(deep_table, flat_local, m.out_bf16)  # [W*n_own, D]
        wide_partial = ops.emb_gather_sum(
            wide_table, flat_local.reshape(W * B, m.f_own), m.out_bf16)

        # ---- route vectors back -----------------------------------------
        vec_recv = torch.empty(B * m.F * D, dtype=vec.dtype, device=device)
        with commprobe.span("a2a_vec"):
            _all_to_all_single(
                vec_recv, vec.reshape(-1),
                [B * len(m.feats_of[s]) * D for s in range(W)],
                [n_own * D] * W, m.group)
        # assemble [B, F, D] (perm feature order) into the MLP input slice
        pos = 0
        target = deep_out_buf[:, col_offset:col_offset + m.F * D] \
            .reshape(B, m.F, D)
        off = 0
        for s in range(W):
            f_s = len(m.feats_of[s])
            chunk = vec_recv[off:off + B * f_s * D].reshape(B, f_s, D)
            target[:, pos:pos + f_s, :] = chunk
            pos += f_s
            off += B * f_s * D

        wide_recv = torch.empty(W * B, dtype=wide_partial.dtype,
                                device=device)
        with commprobe.span("a2a_wide"):
            _all_to_all_single(wide_recv, wide_partial.reshape(-1),
                               [B] * W, [B] * W, m.group)
        wide_out = wide_recv.reshape(W, B).sum(dim=0)

        ctx.module = m
        ctx.save_for_backward(flat_local)
        ctx.local_only = False
        ctx.B = B
        ctx.mark_dirty(deep_out_buf)
        return deep_out_buf, wide_out

    @staticmethod
    def backward(ctx, grad_deep_buf, grad_wide):
        m: "ShardedCriteoEmbeddings" = ctx.module
        (flat_ids,) = ctx.saved_tensors
        W, D = m.world, m.dim
        # grad_deep_buf is the WHOLE MLP-input grad; the embedding slice
        # starts at the col_offset recorded by the module
        col_offset = m._last_col_offset
        emb_grad = grad_deep_buf[:, col_offset:]
        if ctx.local_only:
            # The fused deep+wide SGD kernel reads the column slice where
            # it lies (no 54 MB gather copy per step at the bench shape);
            # every other consumer gets a dense [B, F*D] array.
            if not (emb_grad.is_cuda and ops.HAVE_EXT and D % 4 == 0
                    and emb_grad.stride(1) == 1 and not m._stateful()
                    and emb_grad.dtype == grad_wide.dtype):
                emb_grad = emb_grad.contiguous()
            if ctx.raw_ids:  # [B, F] raw ids: the apply adds the offsets
                m._raw_ids_keys.add(flat_ids.data_ptr())
            m._deep_sink.append((flat_ids, emb_grad))
            m._wide_sink.append((flat_ids, grad_wide.contiguous()))
            return None, None, None, None, None, None, None, None
        B = ctx.B
        n_own = B * m.f_own
        # route deep grads to owners: send chunk for owner s = the
        # features s owns, [B, F_s, D] row-major
        g3 = emb_grad.reshape(B, m.F, D)
        pos = 0
        sends = []
        for s in range(W):
            f_s = len(m.feats_of[s])
            sends.append(g3[:, pos:pos + f_s, :].reshape(-1))
            pos += f_s
        g_send = torch.cat(sends)
        g_recv = torch.empty(W * n_own * D, dtype=g_send.dtype,
                             device=g3.device)
        with commprobe.span("a2a_grad"):
            _all_to_all_single(
                g_recv, g_send, [n_own * D] * W,
                [B * len(m.feats_of[s]) * D for s in range(W)], m.group)
        m._deep_sink.append((flat_ids, g_recv.reshape(W * n_own, D)))
        # wide: every owner needs every rank's grad_wide [B]
        gw = grad_wide.contiguous().reshape(-1)
        gw_all = torch.empty(W * B, dtype=gw.dtype, device=gw.device)
        with commprobe.span("ag_wide"):
            dist.all_gather_into_tensor(gw_all, gw, group=m.group)
        m._wide_sink.append((flat_ids, gw_all))
        return None, None, None, None, None, None, None, None


class ShardedCriteoEmbeddings(SparseOptimizerMixin, nn.Module):
    """Deep (dim-D) + wide (dim-1) categorical embeddings, feature-sharded
    across the process group.  ``forward(ids, deep_out_buf, col_offset)``
    fills ``deep_out_buf[:, col_offset:]`` with [B, F*D] (owner-permuted
    feature order, consistent across steps) and returns the wide sums [B].

    ``sparse_optimizer`` / ``wide_sparse_optimizer`` (None: the same)
    pick the owner-local update rule per table: ``"adagrad"`` keeps
    ``state_sum`` / ``wide_state_sum``, ``"ftrl"`` keeps ``ftrl_accum`` +
    ``ftrl_linear`` / ``wide_ftrl_accum`` + ``wide_ftrl_linear`` (per rank
    like the tables; a table owns state for its own rule only).
    ``sparse_optimizer="rowwise_adagrad"`` keeps ``state_sum_row``, one
    value per owned deep row, and defaults the wide table to
    ``"adagrad"``; it is not a rule for the dim-1 wide table.
    ``"lazy_adam"`` keeps ``adam_exp_avg`` + ``adam_exp_avg_sq`` +
    ``adam_step`` / ``wide_adam_...`` (betas: ``sparse_betas``; each table
    counts its own updates).
    ``sparse_l1`` / ``sparse_l2`` regularise FTRL, ``wide_sparse_lr``
    fixes the wide table's lr.  The binned scatter and its forward-time
    permutation prefetch are SGD-only and run only when both tables are
    ``"sgd"``.
    """

    def __init__(self, table_sizes: List[int], dim: int,
                 out_bf16: bool = False, process_group=None,
                 init_std: Optional[float] = None,
                 wide_init_std: float = 0.01,
                 sparse_optimizer: str = "sgd", sparse_eps: float = 1e-10,
                 sparse_initial_accumulator: float = 0.0,
                 wide_sparse_optimizer: Optional[str] = None,
                 sparse_l1: float = 0.0, sparse_l2: float = 0.0,
                 wide_sparse_lr: Optional[float] = None,
                 sparse_betas: Tuple[float, float] = (0.9, 0.999)):
        super().__init__()
        import math
        self.F = len(table_sizes)
        self.dim = dim
        self.out_bf16 = out_bf16
        self.group = process_group
        self.world, self.rank = _world_rank(process_group)
        W = self.world
        self.feats_of = [[f for f in range(self.F) if f % W == s]
                         for s in range(W)]
        self.own_feats = self.feats_of[self.rank]
        self.f_own = len(self.own_feats)
        own_sizes = [table_sizes[f] for f in self.own_feats]
        total_own = sum(own_sizes)
        std = init_std if init_std is not None else 1.0 / math.sqrt(dim)
        self.weight = nn.Parameter(torch.randn(total_own, dim) * std)
        self.weight._miyarn_sparse = True
        self.weight._miyarn_sharded = True  # never broadcast/replicate
        self.wide_weight = nn.Parameter(
            torch.randn(total_own, 1) * wide_init_std)
        self.wide_weight._miyarn_sparse = True
        self.wide_weight._miyarn_sharded = True
        if wide_sparse_optimizer is None:
            wide_sparse_optimizer = _default_wide_rule(sparse_optimizer)
        self.sparse_optimizer = sparse_optimizer
        self.wide_sparse_optimizer = wide_sparse_optimizer
        self._init_sparse_optimizer(
            sparse_eps, sparse_initial_accumulator,
            {"": (self.weight, sparse_optimizer),
             "wide_": (self.wide_weight, wide_sparse_optimizer)},
            sparse_l1=sparse_l1, sparse_l2=sparse_l2,
            wide_sparse_lr=wide_sparse_lr, sparse_betas=sparse_betas)
        offs = torch.tensor(
            [0] + list(torch.cumsum(torch.tensor(own_sizes), 0)[:-1]),
            dtype=torch.int64)
        # PER-RANK buffers (different size/content on each rank): they must
        # never be broadcast by the reducer — flagged _miyarn_sharded,
        # which BucketedDataParallel skips.
        offs._miyarn_sharded = True
        self.register_buffer("own_offsets", offs, persistent=True)
        # full offsets for the W == 1 local path (perm == identity there)
        full = torch.tensor(
            [0] + list(torch.cumsum(torch.tensor(table_sizes), 0)[:-1]),
            dtype=torch.int64)
        self.register_buffer("full_offsets", full, persistent=True)
        tiled0 = torch.empty(0, dtype=torch.int64)
        tiled0._miyarn_sharded = True
        self.register_buffer("own_offsets_tiled", tiled0,
                             persistent=False)
        self._deep_sink: List[Tuple[torch.Tensor, torch.Tensor]] = []
        self._wide_sink: List[Tuple[torch.Tensor, torch.Tensor]] = []
        self._last_col_offset = 0
        # data_ptr of sink entries that hold RAW [B, F] ids (W == 1 fused
        # lookup): the fused scatter adds full_offsets in the kernel
        self._raw_ids_keys: set = set()
        self._perm_stream = None  # side stream for async pass A
        self._pending_perm = None  # (ids data_ptr, (order, starts), event)
        self._binned_auto: Optional[bool] = None  # skew probe result

    def _ensure_tiled(self, numel: int, device) -> None:
        if self.own_offsets_tiled.numel() < numel:
            reps = (numel + self.f_own - 1) // self.f_own
            tiled = self.own_offsets.to(device).repeat(reps)[:numel]
            tiled._miyarn_sharded = True  # per-rank: never broadcast
            self.own_offsets_tiled = tiled

    def forward(self, ids: torch.Tensor, deep_out_buf: torch.Tensor,
                col_offset: int, dense: Optional[torch.Tensor] = None
                ) -> Tuple[torch.Tensor, torch.Tensor]:
        """Returns (deep_buf_with_grad_fn, wide_sums [B]).  Downstream
        code MUST use the returned buffer (it carries the autograd
        edge).  With ``dense`` (``[B, n_dense]``, ``n_dense <=
        col_offset``, in the buffer's dtype) the columns in front of the
        slice are written here too: ``dense``, then zeros up to
        ``col_offset``; without it they are the caller's."""
        self._last_col_offset = col_offset
        if self.world > 1:
            self._ensure_tiled(self.world * ids.shape[0] * self.f_own,
                               ids.device)
        else:
            self._ensure_tiled(ids.numel(), ids.device)
        out_buf, wide = _ShardedLookup.apply(
            self.weight, self.wide_weight, self, ids, deep_out_buf,
            col_offset, dense, torch.is_grad_enabled())
        return out_buf, wide

    def _fused_lookup_ok(self, ids, dense, deep_out_buf,
                         col_offset: int) -> bool:
        """The W == 1 forward runs as ``ops.emb_lookup_fused``'s single
        kernel (MIYARN_FUSED_LOOKUP=0: never)."""
        return (ops.fused_lookup_enabled()
                and (deep_out_buf.dtype == torch.bfloat16) == self.out_bf16
                and ops.emb_lookup_fused_covers(
                    self.weight, ids, dense, deep_out_buf, col_offset))

    def _scatter_takes_raw_ids(self) -> bool:
        """Whether this step's update will be the fused deep+wide SGD
        scatter, which takes raw ``[B, F]`` ids plus ``full_offsets``:
        both tables on SGD at one lr, and not the binned scatter.  In
        the auto mode the one-time skew probe looks at the flat ids of the
        first training forward; until it has decided, flat ids are
        kept."""
        if self._stateful() or self.wide_sparse_lr is not None \
                or self.dim % 4 != 0:
            return False
        if self.dim != 16:  # the binned scatter is a dim-16 kernel
            return True
        mode = _binned_mode()
        if mode != "auto":
            return mode == "off"
        return self._binned_auto is False

    @torch.no_grad()
    def apply_sparse_updates(self, lr: float, stream=None) -> None:
        """Owner-local fused scatter+SGD (or sparse Adagrad, see
        ``sparse_optimizer``); scale 1/world (grads come from a
        global-mean loss split across ranks).

        ``stream``: optional side HIP stream.  The scatters are atomic-
        bound (memory-side request rate, CUs mostly idle), so running
        them concurrently with the dense optimizer step hides most of
        their latency; the
        CALLER must make the compute stream wait on ``stream`` before the
        next forward's gather reads the tables."""
        if stream is not None:
            stream.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(stream):
                for flat_ids, grad in self._deep_sink:
                    flat_ids.record_stream(stream)
                    grad.record_stream(stream)
                for flat_ids, gw in self._wide_sink:
                    flat_ids.record_stream(stream)
                    gw.record_stream(stream)
                self._apply_pending(lr)
            return
        self._apply_pending(lr)

    def _start_perm_async(self, flat_ids: torch.Tensor,
                          grad_enabled: bool) -> None:
        """Kick off the binned-scatter permutation (pass A) on a side
        stream DURING FORWARD: it depends only on the ids, and its
        ~200 us of latency/atomic-bound work hides under the MFMA-bound
        MLP GEMMs instead of sitting on the backward critical path.
        ``grad_enabled`` is the grad mode of the module's forward call
        (inside ``_ShardedLookup.forward`` autograd has switched it off):
        only a forward that a backward can follow starts one.  An older
        permutation that was never applied is dropped."""
        self._pending_perm = None
        if self._stateful():
            return  # the binned scatter is an SGD kernel
        if not (flat_ids.is_cuda and self.dim == 16 and ops.HAVE_EXT
                and grad_enabled and self._binned_on(flat_ids)):
            return
        rb = ops.pick_region_bits(self.weight.shape[0], flat_ids.numel())
        if not _perm_stream_enabled():
            # inline (A/B diagnostic): pass A runs on the main stream
            perm = ops.binned_permutation(flat_ids, self.weight.shape[0],
                                          rb)
            self._pending_perm = (flat_ids.data_ptr(), perm, None)
            return
        if self._perm_stream is None:
            self._perm_stream = torch.cuda.Stream()
        self._perm_stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(self._perm_stream):
            flat_ids.record_stream(self._perm_stream)
            perm = ops.binned_permutation(flat_ids, self.weight.shape[0],
                                          rb)
        ev = torch.cuda.Event()
        ev.record(self._perm_stream)
        self._pending_perm = (flat_ids.data_ptr(), perm, ev)

    def _binned_on(self, flat_ids: torch.Tensor) -> bool:
        """Resolve the binned-vs-atomic choice (see ``_binned_mode``)."""
        mode = _binned_mode()
        if mode == "on":
            return True
        if mode == "off":
            return False
        if self._binned_auto is None:
            n = flat_ids.numel()
            if n == 0:
                return False
            uniq = int(torch.unique(flat_ids).numel())
            dup = n / max(1, uniq)
            self._binned_auto = dup >= SKEW_THRESHOLD
            logger.info(
                "sparse scatter auto-select: duplication factor %.2f -> "
                "%s path", dup,
                "binned-dedup" if self._binned_auto else "atomic")
        return self._binned_auto

    def _stateful(self) -> bool:
        return (self.sparse_optimizer, self.wide_sparse_optimizer) != \
            ("sgd", "sgd")

    def _apply_pending_stateful(self, lr: float) -> None:
        """Owner-local update when at least one table has a stateful rule
        (Adagrad, FTRL, lazy Adam, row-wise Adagrad).  Deep and wide sink
        entries that share their flat ids go to ``ops.emb_bwd_sparse`` as one pair when
        both rules are stateful: it runs the pair's fused deep+wide kernel
        where there is one (ids read once per pass, one claim per row for
        both tables) and the two single-table updates otherwise.  An SGD
        side is applied here, next to a single-table stateful call.  The
        binned scatter is never used here."""
        scale = 1.0 / self.world
        deep_rule, wide_rule = (self.sparse_optimizer,
                                self.wide_sparse_optimizer)
        wide_lr = lr if self.wide_sparse_lr is None else self.wide_sparse_lr
        deep, wide = self.weight.data, self.wide_weight.data
        if deep_rule == "sgd":
            deep_ws, wide_ws = None, self._adagrad_workspace(wide)
        elif wide_rule == "sgd":
            deep_ws, wide_ws = self._adagrad_workspace(deep), None
        else:
            deep_ws = self._adagrad_workspace(deep, wide)
            wide_ws = deep_ws.wide_view()
        both_stateful = "sgd" not in (deep_rule, wide_rule)
        wide_by_ids = {gw_ids.data_ptr(): (i, gw)
                       for i, (gw_ids, gw) in enumerate(self._wide_sink)}
        paired_wide_done = set()
        for flat_ids, grad in self._deep_sink:
            grad2d = grad.reshape(flat_ids.numel(), self.dim)
            mate = wide_by_ids.get(flat_ids.data_ptr())
            if (both_stateful and mate is not None
                    and mate[0] not in paired_wide_done):
                ops.emb_bwd_sparse(
                    flat_ids,
                    deep=self._sparse_side(deep_rule, "", deep, grad2d, lr),
                    wide=self._sparse_side(wide_rule, "wide_", wide,
                                           mate[1], wide_lr),
                    scale=scale, workspace=deep_ws)
                paired_wide_done.add(mate[0])
            elif deep_rule == "sgd":
                ops.emb_bwd_sgd(deep, flat_ids, grad2d, lr=lr, scale=scale)
            else:
                self._sparse_apply_one(deep_rule, "", deep, flat_ids,
                                       grad2d, lr, scale, deep_ws,
                                       wide=False)
        self._deep_sink.clear()
        for i, (flat_ids, gw) in enumerate(self._wide_sink):
            if i in paired_wide_done:
                continue
            if wide_rule == "sgd":
                fan = self.F if self.world == 1 else self.f_own
                ops.emb_scatter_sum(wide, flat_ids.reshape(gw.numel(), fan),
                                    gw, alpha=-wide_lr * scale)
            else:
                self._sparse_apply_one(wide_rule, "wide_", wide, flat_ids,
                                       gw, wide_lr, scale, wide_ws,
                                       wide=True)
        self._wide_sink.clear()

    def _apply_pending(self, lr: float) -> None:
        if self._stateful():
            self._apply_pending_stateful(lr)
            return
        scale = 1.0 / self.world
        wide_lr = lr if self.wide_sparse_lr is None else self.wide_sparse_lr
        # Binned scatter (round-2 kernel): one region-binned permutation
        # shared by the deep and wide updates (identical flat ids), LDS
        # dedup + exclusive-owner writeback instead of 27M random global
        # atomics.  MIYARN_BINNED_SCATTER=0 restores the atomic kernels
        # for A/B runs.
        first_ids = self._deep_sink[0][0] if self._deep_sink else None
        use_binned = (self.weight.is_cuda and self.dim == 16
                      and ops.HAVE_EXT and first_ids is not None
                      and self._binned_on(first_ids))
        perms = {}
        if use_binned and self._pending_perm is not None:
            key, perm, ev = self._pending_perm
            if ev is not None:
                torch.cuda.current_stream().wait_event(ev)
            # built on the side stream or (inline) on the forward's, used
            # on this one, which may be the caller's ``stream=``: keep the
            # allocator from handing the blocks out while pass B reads them
            for t in perm:
                t.record_stream(torch.cuda.current_stream())
            perms[key] = perm
            self._pending_perm = None

        def perm_for(flat_ids):
            key = flat_ids.data_ptr()
            if key not in perms:
                rb = ops.pick_region_bits(self.weight.shape[0],
                                          flat_ids.numel())
                perms[key] = ops.binned_permutation(
                    flat_ids, self.weight.shape[0], rb)
            return perms[key]

        # Atomic fast path: deep+wide updates share the same flat ids, so
        # one fused kernel reads the ids once and issues both scatters
        # (saves the wide kernel's launch + its 13.6 MB id re-read).
        wide_by_ids = {gw_ids.data_ptr(): (i, gw)
                       for i, (gw_ids, gw) in enumerate(self._wide_sink)}
        fused_wide_done = set()
        raw_keys = self._raw_ids_keys

        def flat_of(ids):
            # raw [B, F] ids that did not get the fused kernel after all
            if ids.data_ptr() in raw_keys and ids.dim() == 2:
                return (ids + self.full_offsets.unsqueeze(0)).reshape(-1)
            return ids

        for flat_ids, grad in self._deep_sink:
            key = flat_ids.data_ptr()
            mate = wide_by_ids.get(key)
            if (not use_binned
                    and mate is not None and flat_ids.is_cuda and ops.HAVE_EXT
                    and self.dim % 4 == 0 and wide_lr == lr
                    and grad.dtype == mate[1].dtype
                    and mate[0] not in fused_wide_done):
                # grad may be the strided slice backward stashed (W == 1)
                ops.emb_bwd_sgd_fused_wide(
                    self.weight.data, self.wide_weight.data, flat_ids,
                    grad, mate[1], lr=lr, scale=scale,
                    offsets=self.full_offsets if key in raw_keys else None)
                fused_wide_done.add(mate[0])
                continue
            flat_ids = flat_of(flat_ids)
            # (a strided slice is gathered into a dense array here)
            grad2d = grad.reshape(flat_ids.numel(), self.dim)
            if use_binned:
                ops.emb_bwd_sgd_binned(
                    self.weight.data, flat_ids, grad2d,
                    lr=lr, scale=scale, perm=perm_for(flat_ids))
            else:
                ops.emb_bwd_sgd(self.weight.data, flat_ids, grad2d,
                                lr=lr, scale=scale)
        self._deep_sink.clear()
        for i, (flat_ids, gw) in enumerate(self._wide_sink):
            if i in fused_wide_done:
                continue
            flat_ids = flat_of(flat_ids)
            # gw layout [W, B] (or [B] local); ids layout [peer][b][j]
            if use_binned:
                ops.emb_scatter_sum_binned(
                    self.wide_weight.data, flat_ids, gw,
                    alpha=-wide_lr * scale, perm=perm_for(flat_ids))
                continue
            fan = self.F if self.world == 1 else self.f_own
            ids2d = flat_ids.reshape(gw.numel(), fan)
            ops.emb_scatter_sum(self.wide_weight.data, ids2d, gw,
                                alpha=-wide_lr * scale)
        self._wide_sink.clear()
        raw_keys.clear()

    def clear_pending(self) -> None:
        self._deep_sink.clear()
        self._wide_sink.clear()
        self._raw_ids_keys.clear()
        # matched to its ids by address: must not outlive them
        self._pending_perm = None
