"""recommender_system_amd — MI355X-native CTR forward path.

Drop-in for the embedding-lookup + feature-interaction forward path of
Hcyand/recommender_system (FM second order, PNN inner product, DCN CrossNet,
DIN attention), as hand-written gfx950 HIP kernels behind a C-ABI
(include/rs_capi.h, librs_hip.so) with a Python host layer that keeps the
reference's Keras layer / model names and signatures.
"""
from . import _lib, metrics, optim  # noqa: F401
from .layers import (AFMLayer, Attention, AttentionLayer, BatchNormalization, CrossLayer, Dense, Dice,  # noqa: F401
                     DNNLayer, EmbedLayer, FFMLayer, FGCNNLayer, FMLayer, InnerProductLayer, InteractionLayer,
                     OuterProductLayer, ResLayer, WideLayer, mmoe_layer, sigmoid_combine, tower_layer,
                     AUGRU, AUGRUCell, AttentionSequencePoolingLayer, DNN, GRU, InterestEvolution,
                     LocalActivationUnit, PredictionLayer, InBatchSoftmaxLayer, SequencePoolingLayer)
from .models import AFM, DCN, DIEN, DIN, DSSM, FFM, FM, FNN, MMOE, NFM, PNN, DeepCrossing, DeepFM, WideDeep  # noqa: F401
from .feature_column import DenseFeat, SparseFeat, VarLenSparseFeat, get_feature_names  # noqa: F401
from .negative import NegativeSampler, recall_N, sampledsoftmaxloss  # noqa: F401
from .metrics import BinaryMetrics, binary_metrics, group_auc, roc_auc  # noqa: F401
from .retrieval import topn_inner_product, topn_ok  # noqa: F401
from .dataset import create_criteo_dataset, denseFeature, features_dict, sparseFeature  # noqa: F401

__version__ = "0.1.0"
