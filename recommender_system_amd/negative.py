"""Negative-sampling helpers of the retrieval models (DSSM) — the
reference's utils/negative.py:18-54 without TensorFlow:

  NegativeSampler(sampler, num_sampled, item_name, item_count=None,
                  distortion=1.0)    the same namedtuple and validation
  sampledsoftmaxloss(y_true, y_pred) the mean of the model's per-sample loss
  recall_N(y_true, y_pred, N=50)

(``check_version`` — a query of a package index over the network — has no
counterpart here.)
"""
from __future__ import annotations

from collections import namedtuple


class NegativeSampler(namedtuple("NegativeSampler", ["sampler", "num_sampled", "item_name", "item_count",
                                                     "distortion"])):
    """sampler: 'inbatch', 'uniform', 'frequency' or 'adaptive'; num_sampled:
    negatives per positive; item_name: the item tower's key feature;
    item_count: global frequency of every item; distortion: skew of the
    unigram distribution."""
    __slots__ = ()

    def __new__(cls, sampler, num_sampled, item_name, item_count=None, distortion=1.0):
        if sampler not in ["inbatch", "uniform", "frequency", "adaptive"]:
            raise ValueError(" `%s` sampler is not supported " % sampler)
        if sampler in ["inbatch", "frequency"] and item_count is None:
            raise ValueError(" `item_count` must not be `None` when using `inbatch` or `frequency` sampler")
        return super().__new__(cls, sampler, num_sampled, item_name, item_count, distortion)


def sampledsoftmaxloss(y_true, y_pred):
    """K.mean(y_pred): the model's output already is the per-sample loss."""
    return y_pred.mean()


def recall_N(y_true, y_pred, N=50):
    return len(set(y_pred[:N]) & set(y_true)) * 1.0 / len(y_true)
