"""Feature columns of the DeepCTR-style models (DIEN) — the reference's
utils/feature_column.py:12-116 as plain namedtuples: same fields, order and
defaults, no TensorFlow objects.

  SparseFeat(name, vocabulary_size, embedding_dim=4, use_hash=False,
             vocabulary_path=None, dtype='int32', embeddings_initializer=None,
             embedding_name=None, group_name='default_group', trainable=True)
  VarLenSparseFeat(sparsefeat, maxlen, combiner='mean', length_name=None,
                   weight_name=None, weight_norm=True)
  DenseFeat(name, dimension=1, dtype='float32', transform_fn=None)
  get_feature_names(feature_columns)

``embeddings_initializer=None`` stands for the reference's default,
RandomNormal(mean 0, stddev 1e-4); a callable ``f(shape, generator) -> tensor``
replaces it.  ``embedding_dim='auto'`` is 6 * int(vocabulary_size ** 0.25) and
``embedding_name`` defaults to the feature's name, as in the reference.  Not
built: ``use_hash=True``, ``weight_name`` and ``transform_fn`` raise
NotImplementedError where the column is created.
"""
from __future__ import annotations

from collections import OrderedDict, namedtuple

DEFAULT_GROUP_NAME = "default_group"


class SparseFeat(namedtuple("SparseFeat", ["name", "vocabulary_size", "embedding_dim", "use_hash", "vocabulary_path",
                                           "dtype", "embeddings_initializer", "embedding_name", "group_name",
                                           "trainable"])):
    __slots__ = ()

    def __new__(cls, name, vocabulary_size, embedding_dim=4, use_hash=False, vocabulary_path=None, dtype="int32",
                embeddings_initializer=None, embedding_name=None, group_name=DEFAULT_GROUP_NAME, trainable=True):
        if use_hash:
            raise NotImplementedError("SparseFeat: use_hash=True (hashed ids) is not built")
        if embedding_dim == "auto":
            embedding_dim = 6 * int(pow(vocabulary_size, 0.25))
        if embedding_name is None:
            embedding_name = name
        return super().__new__(cls, name, vocabulary_size, embedding_dim, use_hash, vocabulary_path, dtype,
                               embeddings_initializer, embedding_name, group_name, trainable)

    def __hash__(self):
        return self.name.__hash__()


class VarLenSparseFeat(namedtuple("VarLenSparseFeat", ["sparsefeat", "maxlen", "combiner", "length_name",
                                                       "weight_name", "weight_norm"])):
    __slots__ = ()

    def __new__(cls, sparsefeat, maxlen, combiner="mean", length_name=None, weight_name=None, weight_norm=True):
        if weight_name is not None:
            raise NotImplementedError("VarLenSparseFeat: weight_name (weighted sequences) is not built")
        return super().__new__(cls, sparsefeat, maxlen, combiner, length_name, weight_name, weight_norm)

    name = property(lambda self: self.sparsefeat.name)
    vocabulary_size = property(lambda self: self.sparsefeat.vocabulary_size)
    embedding_dim = property(lambda self: self.sparsefeat.embedding_dim)
    use_hash = property(lambda self: self.sparsefeat.use_hash)
    vocabulary_path = property(lambda self: self.sparsefeat.vocabulary_path)
    dtype = property(lambda self: self.sparsefeat.dtype)
    embeddings_initializer = property(lambda self: self.sparsefeat.embeddings_initializer)
    embedding_name = property(lambda self: self.sparsefeat.embedding_name)
    group_name = property(lambda self: self.sparsefeat.group_name)
    trainable = property(lambda self: self.sparsefeat.trainable)

    def __hash__(self):
        return self.name.__hash__()


class DenseFeat(namedtuple("DenseFeat", ["name", "dimension", "dtype", "transform_fn"])):
    __slots__ = ()

    def __new__(cls, name, dimension=1, dtype="float32", transform_fn=None):
        if transform_fn is not None:
            raise NotImplementedError("DenseFeat: transform_fn is not built")
        return super().__new__(cls, name, dimension, dtype, transform_fn)

    def __hash__(self):
        return self.name.__hash__()


def build_input_features(feature_columns):
    """name -> column (or the string 'length' for a length input), in the
    reference's input order: each column's name, a var-len column's length_name
    right after it (once)."""
    features = OrderedDict()
    for fc in feature_columns:
        if isinstance(fc, (SparseFeat, DenseFeat)):
            features[fc.name] = fc
        elif isinstance(fc, VarLenSparseFeat):
            features[fc.name] = fc
            if fc.length_name is not None:
                features[fc.length_name] = "length"
        else:
            raise TypeError("Invalid feature column type,got", type(fc))
    return features


def get_feature_names(feature_columns):
    return list(build_input_features(feature_columns).keys())
