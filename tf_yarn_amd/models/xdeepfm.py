"""xDeepFM for Criteo, on the same embedding modules as wide-and-deep, DLRM,
DCN and AutoInt.

``bottom MLP(dense) -> [B, D]`` is field 0 and one :class:`SparseEmbedding`
lookup gives fields ``1..F``: ``x0 [B, m*D]``, ``m = F + 1``.  A Compressed
Interaction Network of ``len(cin)`` layers (:func:`tf_yarn_amd.ops.cin_layer`:
one MFMA kernel forward, two backward in bf16 on the GPU; the ``[B, H*m, D]``
outer product is never formed) crosses every feature map of the previous
layer with every field of ``x0``; each layer's maps are sum-pooled over the
embedding axis, and the pooled features join an MLP over ``x0`` under one
single-logit head.  The tables are replicated; every sparse rule and the
multi-hot bags of :class:`SparseEmbedding` apply unchanged, and the sparse
sync methods have :class:`WideAndDeep`'s signatures, so the same training
loops drive it.  The linear term of the paper and sharded tables are not
offered.
"""

from __future__ import annotations

import math
from typing import List, Optional, Sequence, Tuple

import torch
from torch import nn

from tf_yarn_amd import ops
from tf_yarn_amd.models.dlrm import DLRM, _mlp
from tf_yarn_amd.models.wide_deep import (CRITEO_DENSE, DEFAULT_TABLE_SIZES,
                                          ScalarHead, SparseEmbedding)


class CINLayer(nn.Module):
    """``forward(x0 [B, m*D], x [B, h_in*D]) -> [B, h_out*D]``, the linear
    CIN layer ``y[b,h,c] = sum_ij weight[h,i,j] * x[b,i,c] * x0[b,j,c]``
    through :func:`ops.cin_layer`."""

    def __init__(self, h_in: int, n_fields: int, h_out: int,
                 dtype=torch.float32):
        super().__init__()
        self.n_fields = n_fields
        self.weight = nn.Parameter(
            torch.empty(h_out, h_in, n_fields, dtype=dtype))
        # a [h_out, h_in * m] linear map: fan-in h_in * m
        nn.init.kaiming_uniform_(self.weight.view(h_out, -1), a=math.sqrt(5))

    def forward(self, x0: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
        return ops.cin_layer(x0, x, self.weight, self.n_fields)


class CIN(nn.Module):
    """``forward(x0 [B, m*D]) -> [B, sum(widths)]`` fp32: the layers of
    ``widths`` feature maps, starting from ``x = x0``, each sum-pooled over
    the embedding axis."""

    def __init__(self, n_fields: int, widths: Sequence[int],
                 dtype=torch.float32):
        super().__init__()
        self.n_fields = n_fields
        self.widths = tuple(widths)
        self.layers = nn.ModuleList(
            CINLayer(h_in, n_fields, h_out, dtype)
            for h_in, h_out in zip((n_fields,) + self.widths, self.widths))

    def forward(self, x0: torch.Tensor) -> torch.Tensor:
        b, x, pooled = x0.shape[0], x0, []
        for layer, h in zip(self.layers, self.widths):
            x = layer(x0, x)
            pooled.append(x.view(b, h, -1).float().sum(-1))
        return torch.cat(pooled, dim=1)


class XDeepFM(nn.Module):
    """Compressed interaction network plus an MLP over the embeddings."""

    DENSE_ALIGN = DLRM.DENSE_ALIGN

    def __init__(self,
                 dense_dim: int = CRITEO_DENSE,
                 table_sizes: Optional[List[int]] = None,
                 embedding_dim: int = 16,
                 bottom: Tuple[int, ...] = (512, 256),
                 cin: Tuple[int, ...] = (128, 128),
                 deep: Tuple[int, ...] = (400, 400),
                 compute_dtype: torch.dtype = torch.float32,
                 combiner: str = "sum",
                 sparse_optimizer: str = "sgd",
                 sparse_eps: float = 1e-10,
                 sparse_initial_accumulator: float = 0.0,
                 sparse_l1: float = 0.0, sparse_l2: float = 0.0,
                 sparse_betas: Tuple[float, float] = (0.9, 0.999)):
        """``bottom``: the hidden widths of the bottom MLP, which ends in
        one more layer of width ``embedding_dim`` (field 0); ``cin``: the
        feature maps of each CIN layer; ``deep``: the widths of the MLP over
        the ``m * embedding_dim`` columns of ``x0``, whose output is
        concatenated with the ``sum(cin)`` pooled CIN features under the
        single-logit head.  The sparse arguments and ``combiner`` are
        :class:`SparseEmbedding`'s."""
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
        self.cin = CIN(self.n_fields, cin)
        self.mlp, width = _mlp(self.n_fields * embedding_dim, deep)
        self.head = ScalarHead(width + sum(cin), compute_dtype)
        if bf16:
            # dense compute in bf16; masters are managed by the optimizer
            self.bottom_mlp = self.bottom_mlp.to(torch.bfloat16)
            self.cin = self.cin.to(torch.bfloat16)
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
        x0 = torch.cat([dense_vec, emb], dim=1)
        pooled = self.cin(x0).to(self.compute_dtype)
        logits = self.head(torch.cat([pooled, self.mlp(x0)], dim=1))
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
