"""Deep-and-cross network (DCN-v2, stacked form) for Criteo, on the same
embedding modules as wide-and-deep and DLRM.

``x0 = [dense padded to 16 | embeddings] [B, D]`` is built in one buffer
the way :class:`WideAndDeep` builds its deep input (``_DeepInput`` one-hot,
``ops.EmbeddingBagFn`` writing behind the dense columns multi-hot), then
``n_cross`` cross layers ``x <- x0 * (x @ W^T + b) + x``
(:func:`tf_yarn_amd.ops.cross_layer`: one MFMA kernel forward in bf16 on
the GPU; with ``cross_rank`` the low-rank ``W = U V^T`` of
:func:`tf_yarn_amd.ops.cross_layer_lowrank`), an MLP of Linear + ReLU and a single-logit head.  The tables are
replicated; every sparse rule and the multi-hot bags of
:class:`SparseEmbedding` apply unchanged, and the sparse sync methods have
:class:`WideAndDeep`'s signatures, so the same training loops drive it.
Sharded tables are not offered.
"""

from __future__ import annotations

import math
from typing import List, Optional, Tuple

import torch
from torch import nn

from tf_yarn_amd import ops
from tf_yarn_amd.models.dlrm import _mlp
from tf_yarn_amd.models.wide_deep import (CRITEO_DENSE, DEFAULT_TABLE_SIZES,
                                          BagUpdate, ScalarHead,
                                          SparseEmbedding, _DeepInput)


class CrossLayer(nn.Module):
    """``forward(x0, x) = x0 * (x @ weight.T + bias) + x`` with a full-rank
    ``weight [dim, dim]`` (initialised like ``FusedLinearReLU``'s) and a
    zero ``bias``."""

    def __init__(self, dim: int, dtype=torch.float32):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(dim, dim, dtype=dtype))
        self.bias = nn.Parameter(torch.zeros(dim, dtype=dtype))
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))

    def forward(self, x0: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
        return ops.cross_layer(x0, x, self.weight, self.bias)


class LowRankCrossLayer(nn.Module):
    """``forward(x0, x) = x0 * (u_weight @ (v_weight @ x) + bias) + x``: the
    low-rank cross layer with ``v_weight [rank, dim]`` (down) and
    ``u_weight [dim, rank]`` (up), both initialised like
    :class:`CrossLayer`'s weight, and a zero ``bias``."""

    def __init__(self, dim: int, rank: int, dtype=torch.float32):
        super().__init__()
        self.v_weight = nn.Parameter(torch.empty(rank, dim, dtype=dtype))
        self.u_weight = nn.Parameter(torch.empty(dim, rank, dtype=dtype))
        self.bias = nn.Parameter(torch.zeros(dim, dtype=dtype))
        nn.init.kaiming_uniform_(self.v_weight, a=math.sqrt(5))
        nn.init.kaiming_uniform_(self.u_weight, a=math.sqrt(5))

    def forward(self, x0: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
        return ops.cross_layer_lowrank(x0, x, self.v_weight, self.u_weight,
                                       self.bias)


class CrossNetwork(nn.Module):
    """``n_layers`` cross layers, starting from ``x = x0``: full-rank
    :class:`CrossLayer` s, or :class:`LowRankCrossLayer` s of ``rank``."""

    def __init__(self, dim: int, n_layers: int, dtype=torch.float32,
                 rank: Optional[int] = None):
        super().__init__()
        self.layers = nn.ModuleList(
            CrossLayer(dim, dtype) if rank is None
            else LowRankCrossLayer(dim, rank, dtype)
            for _ in range(n_layers))

    def forward(self, x0: torch.Tensor) -> torch.Tensor:
        x = x0
        for layer in self.layers:
            x = layer(x0, x)
        return x


class DCN(nn.Module):
    """Stacked deep-and-cross network: cross network, then the MLP."""

    def __init__(self,
                 dense_dim: int = CRITEO_DENSE,
                 table_sizes: Optional[List[int]] = None,
                 embedding_dim: int = 16,
                 n_cross: int = 3,
                 deep: Tuple[int, ...] = (1024, 512, 256),
                 compute_dtype: torch.dtype = torch.float32,
                 combiner: str = "sum",
                 sparse_optimizer: str = "sgd",
                 sparse_eps: float = 1e-10,
                 sparse_initial_accumulator: float = 0.0,
                 sparse_l1: float = 0.0, sparse_l2: float = 0.0,
                 sparse_betas: Tuple[float, float] = (0.9, 0.999),
                 cross_rank: Optional[int] = None):
        """``n_cross``: the number of cross layers over the
        ``16 + len(table_sizes) * embedding_dim`` columns of ``x0``;
        ``cross_rank``: ``None`` for full-rank layers, else the rank of
        :class:`LowRankCrossLayer` (about a quarter of the columns);
        ``deep``: the widths of the MLP behind them, which feeds the
        single-logit head.  ``dense_dim`` is at most 16 (the dense columns
        share ``WideAndDeep``'s 16-column slot of the input buffer).  The
        sparse arguments and ``combiner`` are :class:`SparseEmbedding`'s."""
        super().__init__()
        table_sizes = table_sizes or DEFAULT_TABLE_SIZES
        if dense_dim > _DeepInput.DENSE_PAD:
            raise ValueError(
                f"dense_dim {dense_dim} > {_DeepInput.DENSE_PAD}")
        self.compute_dtype = compute_dtype
        self.dense_dim = dense_dim
        self.sparse_optimizer = sparse_optimizer
        self.combiner = combiner
        bf16 = compute_dtype == torch.bfloat16
        self.embedding = SparseEmbedding(
            table_sizes, embedding_dim, out_bf16=bf16, combiner=combiner,
            sparse_optimizer=sparse_optimizer, sparse_eps=sparse_eps,
            sparse_initial_accumulator=sparse_initial_accumulator,
            sparse_l1=sparse_l1, sparse_l2=sparse_l2,
            sparse_betas=sparse_betas)
        dim = _DeepInput.DENSE_PAD + len(table_sizes) * embedding_dim
        self.cross = CrossNetwork(dim, n_cross, rank=cross_rank)
        self.mlp, width = _mlp(dim, deep)
        self.head = ScalarHead(width, compute_dtype)
        if bf16:
            # dense compute in bf16; masters are managed by the optimizer
            self.cross = self.cross.to(torch.bfloat16)
            self.mlp = self.mlp.to(torch.bfloat16)

    def _x0(self, dense, sparse_ids, bag_offsets, sparse_weights):
        emb = self.embedding
        bf16 = self.compute_dtype == torch.bfloat16
        if bag_offsets is not None:
            return ops.EmbeddingBagFn.apply(
                emb.weight, sparse_ids, bag_offsets, len(emb.table_sizes),
                emb.offsets, sparse_weights, self.combiner, bf16, emb._sink,
                dense, _DeepInput.DENSE_PAD, BagUpdate._make)
        flat = (sparse_ids + emb.offsets.unsqueeze(0)).reshape(-1)
        return _DeepInput.apply(dense, emb.weight, flat, emb.dim, bf16,
                                emb._sink)

    def forward(self, dense: torch.Tensor, sparse_ids: torch.Tensor,
                labels: Optional[torch.Tensor] = None,
                bag_offsets: Optional[torch.Tensor] = None,
                sparse_weights: Optional[torch.Tensor] = None
                ) -> torch.Tensor:
        """Logits ``[B]``, or the mean BCE-with-logits loss when ``labels``
        is given.  One-hot: ``sparse_ids [B, F]``; multi-hot:
        ``sparse_ids [nnz]`` with ``bag_offsets [B*F + 1]`` (and optional
        ``sparse_weights [nnz]``), pooled by the model's ``combiner``."""
        if sparse_weights is not None and bag_offsets is None:
            raise ValueError("sparse_weights needs bag_offsets")
        dense = dense.to(self.compute_dtype)
        x0 = self._x0(dense, sparse_ids, bag_offsets, sparse_weights)
        logits = self.head(self.mlp(self.cross(x0)))
        if labels is None:
            return logits
        return nn.functional.binary_cross_entropy_with_logits(
            logits.float(), labels.float())

    def start_sparse_sync(self, process_group=None) -> None:
        self.embedding.start_sparse_sync(process_group)

    def finish_sparse_sync(self, lr: float, stream=None) -> None:
        self.embedding.finish_sparse_sync(lr)

    def apply_sparse_updates(self, lr: float, process_group=None) -> None:
        self.start_sparse_sync(process_group)
        self.finish_sparse_sync(lr)

    def clear_pending(self) -> None:
        self.embedding.clear_pending()
