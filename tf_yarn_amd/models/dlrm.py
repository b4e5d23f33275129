"""DLRM for Criteo, on the same embedding modules as wide-and-deep.

``bottom MLP(dense) -> [B, D]``, one :class:`SparseEmbedding` lookup
``-> [B, F*D]``, the pairwise dot interaction of the ``F + 1`` vectors
(:func:`tf_yarn_amd.ops.dot_interaction`: one HIP kernel forward, one
backward in bf16 on the GPU), the top MLP over its ``W`` columns and a
single-logit head.  The tables are replicated; every sparse rule and the
multi-hot bags of :class:`SparseEmbedding` apply unchanged, and the sparse
sync methods have :class:`WideAndDeep`'s signatures, so the same training
loops drive it.  Sharded tables are not offered.
"""

from __future__ import annotations

from typing import List, Optional, Tuple

import torch
from torch import nn

from tf_yarn_amd import ops
from tf_yarn_amd.models.wide_deep import (CRITEO_DENSE, DEFAULT_TABLE_SIZES,
                                          FusedLinearReLU, ScalarHead,
                                          SparseEmbedding)


def _mlp(in_dim: int, widths) -> Tuple[nn.Sequential, int]:
    layers: List[nn.Module] = []
    for w in widths:
        layers.append(FusedLinearReLU(in_dim, w))
        in_dim = w
    return nn.Sequential(*layers), in_dim


class DLRM(nn.Module):
    """Deep learning recommendation model with the "dot" interaction."""

    # the dense columns are zero-padded to a multiple of this: the fused
    # linear layers want K % 16 == 0
    DENSE_ALIGN = 16

    def __init__(self,
                 dense_dim: int = CRITEO_DENSE,
                 table_sizes: Optional[List[int]] = None,
                 embedding_dim: int = 16,
                 bottom: Tuple[int, ...] = (512, 256),
                 top: Tuple[int, ...] = (1024, 1024, 512, 256),
                 compute_dtype: torch.dtype = torch.float32,
                 combiner: str = "sum",
                 sparse_optimizer: str = "sgd",
                 sparse_eps: float = 1e-10,
                 sparse_initial_accumulator: float = 0.0,
                 sparse_l1: float = 0.0, sparse_l2: float = 0.0,
                 sparse_betas: Tuple[float, float] = (0.9, 0.999)):
        """``bottom``: the hidden widths of the bottom MLP, which ends in
        one more layer of width ``embedding_dim``; ``top``: the widths of
        the top MLP, which reads the interaction's
        ``ops.dot_interaction_width(len(table_sizes), embedding_dim)``
        columns and feeds the single-logit head.  Every layer is Linear +
        ReLU.  The sparse arguments and ``combiner`` are
        :class:`SparseEmbedding`'s."""
        super().__init__()
        table_sizes = table_sizes or DEFAULT_TABLE_SIZES
        self.compute_dtype = compute_dtype
        self.dense_dim = dense_dim
        self.sparse_optimizer = sparse_optimizer
        bf16 = compute_dtype == torch.bfloat16
        self.dense_pad = -dense_dim % self.DENSE_ALIGN
        self.bottom_mlp, _ = _mlp(dense_dim + self.dense_pad,
                                  tuple(bottom) + (embedding_dim,))
        self.embedding = SparseEmbedding(
            table_sizes, embedding_dim, out_bf16=bf16, combiner=combiner,
            sparse_optimizer=sparse_optimizer, sparse_eps=sparse_eps,
            sparse_initial_accumulator=sparse_initial_accumulator,
            sparse_l1=sparse_l1, sparse_l2=sparse_l2,
            sparse_betas=sparse_betas)
        self.top_mlp, width = _mlp(
            ops.dot_interaction_width(len(table_sizes), embedding_dim), top)
        self.head = ScalarHead(width, compute_dtype)
        if bf16:
            # dense compute in bf16; masters are managed by the optimizer
            self.bottom_mlp = self.bottom_mlp.to(torch.bfloat16)
            self.top_mlp = self.top_mlp.to(torch.bfloat16)

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
        if self.dense_pad:
            dense = nn.functional.pad(dense, (0, self.dense_pad))
        dense_vec = self.bottom_mlp(dense)
        emb = self.embedding(sparse_ids, bag_offsets, sparse_weights)
        z = ops.dot_interaction(dense_vec, emb)
        logits = self.head(self.top_mlp(z))
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
