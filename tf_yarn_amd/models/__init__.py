from tf_yarn_amd.models.wide_deep import (CRITEO_DENSE, CRITEO_SPARSE,
                                          SparseEmbedding, WideAndDeep)
from tf_yarn_amd.models.dlrm import DLRM
from tf_yarn_amd.models.dcn import (DCN, CrossLayer, CrossNetwork,
                                    LowRankCrossLayer)
from tf_yarn_amd.models.autoint import AutoInt, FieldAttentionLayer
from tf_yarn_amd.models.xdeepfm import CIN, CINLayer, XDeepFM
from tf_yarn_amd.models.mlp import MLP
from tf_yarn_amd.models.synthetic import (SyntheticCriteoDataset,
                                          SyntheticImageDataset,
                                          synthetic_criteo_batch)

__all__ = ["WideAndDeep", "DLRM", "DCN", "CrossLayer", "CrossNetwork",
           "LowRankCrossLayer",
           "AutoInt", "FieldAttentionLayer", "XDeepFM", "CIN", "CINLayer",
           "SparseEmbedding", "MLP",
           "SyntheticCriteoDataset", "SyntheticImageDataset",
           "synthetic_criteo_batch", "CRITEO_DENSE", "CRITEO_SPARSE"]
