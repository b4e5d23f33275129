"""AutoInt for Criteo, on the same embedding modules as wide-and-deep, DLRM
and DCN.

``bottom MLP(dense) -> [B, D]`` is token 0 and one :class:`SparseEmbedding`
lookup gives tokens ``1..F``; ``n_layers`` interacting layers of multi-head
self-attention over the ``N = F + 1`` tokens of each example
(:func:`tf_yarn_amd.ops.field_attention`: one HIP kernel forward, one
backward in bf16 on the GPU) follow, then an optional MLP over the
``[B, N*H*d]`` result and a single-logit head.  The tables are replicated;
every sparse rule and the multi-hot bags of :class:`SparseEmbedding` apply
unchanged, and the sparse sync methods have :class:`WideAndDeep`'s
signatures, so the same training loops drive it.  Sharded tables are not
offered.
"""

from __future__ import annotations

import math
from typing import List, Optional, Tuple

import torch
from torch import nn

from tf_yarn_amd import ops
from tf_yarn_amd.models.dlrm import DLRM, _mlp
from tf_yarn_amd.models.wide_deep import (CRITEO_DENSE, DEFAULT_TABLE_SIZES,
                                          ScalarHead, SparseEmbedding)


class FieldAttentionLayer(nn.Module):
    """``forward(x [B*N, in_dim], n_fields)`` = ``relu(field_attention(x @
    Wqkv^T) + x @ Wres^T)`` per token, ``[B*N, n_heads * head_dim]``: two
    bias-free projections through torch's linear, the attention through
    :func:`ops.field_attention`, the add and the ReLU in torch."""

    def __init__(self, in_dim: int, n_heads: int, head_dim: int,
                 dtype=torch.float32):
        super().__init__()
        self.n_heads = n_heads
        width = n_heads * head_dim
        self.qkv_weight = nn.Parameter(
            torch.empty(3 * width, in_dim, dtype=dtype))
        self.res_weight = nn.Parameter(torch.empty(width, in_dim, dtype=dtype))
        for w in (self.qkv_weight, self.res_weight):
            nn.init.kaiming_uniform_(w, a=math.sqrt(5))

    def forward(self, x: torch.Tensor, n_fields: int) -> torch.Tensor:
        qkv = nn.functional.linear(x, self.qkv_weight)
        att = ops.field_attention(qkv, n_fields, self.n_heads)
        return torch.relu(att + nn.functional.linear(x, self.res_weight))


class AutoInt(nn.Module):
    """Automatic feature interaction by self-attention over the fields."""

    DENSE_ALIGN = DLRM.DENSE_ALIGN

    def __init__(self,
                 dense_dim: int = CRITEO_DENSE,
                 table_sizes: Optional[List[int]] = None,
                 embedding_dim: int = 16,
                 bottom: Tuple[int, ...] = (512, 256),
                 n_layers: int = 3,
                 n_heads: int = 2,
                 head_dim: int = 16,
                 deep: Tuple[int, ...] = (),
                 compute_dtype: torch.dtype = torch.float32,
                 combiner: str = "sum",
                 sparse_optimizer: str = "sgd",
                 sparse_eps: float = 1e-10,
                 sparse_initial_accumulator: float = 0.0,
                 sparse_l1: float = 0.0, sparse_l2: float = 0.0,
                 sparse_betas: Tuple[float, float] = (0.9, 0.999)):
        """``bottom``: the hidden widths of the bottom MLP, which ends in
        one more layer of width ``embedding_dim`` (token 0); ``n_layers``
        attention layers of ``n_heads`` heads of ``head_dim``; ``deep``: the
        widths of the MLP between the ``N * n_heads * head_dim`` attention
        columns and the single-logit head (none by default).  The sparse
        arguments and ``combiner`` are :class:`SparseEmbedding`'s."""
        super().__init__()
        table_sizes = table_sizes or DEFAULT_TABLE_SIZES
        self.compute_dtype = compute_dtype
        self.dense_dim = dense_dim
        self.sparse_optimizer = sparse_optimizer
        self.n_fields = len(table_sizes) + 1
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
        width = n_heads * head_dim
        self.layers = nn.ModuleList(
            FieldAttentionLayer(embedding_dim if i == 0 else width, n_heads,
                                head_dim)
            for i in range(n_layers))
        self.mlp, width = _mlp(self.n_fields * width, deep)
        self.head = ScalarHead(width, compute_dtype)
        if bf16:
            # dense compute in bf16; masters are managed by the optimizer
            self.bottom_mlp = self.bottom_mlp.to(torch.bfloat16)
            self.layers = self.layers.to(torch.bfloat16)
            self.mlp = self.mlp.to(torch.bfloat16)

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
        n = self.n_fields
        x = torch.cat([dense_vec, emb], dim=1).reshape(
            dense_vec.shape[0] * n, -1)
        for layer in self.layers:
            x = layer(x, n)
        logits = self.head(self.mlp(x.reshape(dense_vec.shape[0], -1)))
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
