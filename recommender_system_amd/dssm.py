"""DSSM — the reference's two-tower retrieval model (model/dssm.py:17-90),
forward.  ``models.DSSM`` is this class."""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from ._lib import call, ptr
from ._train_ops import _subseed
from .feature_column import DenseFeat, SparseFeat, VarLenSparseFeat, build_input_features
from .layers import (DNN, InBatchSoftmaxLayer, KerasModule, TowerMixin, _ErrFlag, _ids_tensor, _lengths,
                     _to_device_f32, l2_normalize, seq_pool, seq_pool_arrays, seq_pool_ok, _SEQ_MAXF)

_CC_MAXP = 16  # pieces of rs_concat_pieces / rs_dssm_tower_fwd


class _Tower(TowerMixin, KerasModule):
    """One tower: its columns, their places in the input row, and its DNN."""

    def __init__(self, cols, hidden_units, activation, l2_reg, dropout, use_bn, device, seed):
        super().__init__(device, seed)
        self.features = build_input_features(cols)  # (raises the reference's TypeError on a foreign column)
        self.sparse_cols = [c for c in cols if isinstance(c, SparseFeat)]
        self.varlen_cols = [c for c in cols if isinstance(c, VarLenSparseFeat)]
        self.dense_cols = [c for c in cols if isinstance(c, DenseFeat)]
        for c in self.varlen_cols:
            if c.combiner not in ("sum", "mean", "max"):
                raise ValueError("mode must be sum or mean")
        if not cols:
            raise NotImplementedError("dnn_feature_columns can not be empty list")
        # [SparseFeat rows | pooled var-len features | dense values] (layer/utils.py:140-150)
        col = 0
        self.sparse_at, self.varlen_at, self.dense_at = [], [], []
        for c in self.sparse_cols:
            self.sparse_at.append(col)
            col += c.embedding_dim
        for c in self.varlen_cols:
            self.varlen_at.append(col)
            col += c.embedding_dim
        for c in self.dense_cols:
            self.dense_at.append(col)
            col += c.dimension
        self.input_width = col
        self.dnn = DNN(hidden_units, activation, l2_reg, dropout, use_bn, output_activation="linear", device=device,
                       seed=_subseed(self._gen), input_dim=col)
        self.out_width = self.dnn.hidden_units[-1] if self.dnn.hidden_units else col

    def _layers(self):
        return list(self.dnn.layers)

    def _acts(self):
        return [_lib.ACT.get(l.activation, -1) for l in self.dnn.layers]

    def mlp_ok(self):
        """The tower as one rs_mlp_fwd launch (a BN / Dice tower runs layer by layer)."""
        return bool(self.dnn.layers) and not self.dnn.use_bn and self.tower_ok()

    def fused_ok(self):
        """The whole tower as one rs_dssm_tower_fwd launch."""
        n_seq, n_pc = len(self.varlen_cols), len(self.sparse_cols) + len(self.dense_cols)
        if (self.dnn.use_bn and self.dnn.layers) or n_seq > _SEQ_MAXF:
            return False
        if not all(seq_pool_ok(c.embedding_dim) for c in self.varlen_cols):
            return False
        dims = [self.input_width] + self.dnn.hidden_units
        n = len(self.dnn.layers)
        return bool(_lib.lib().rs_dssm_tower_ok(n_pc + n_seq, n, (C.c_int * (n + 1))(*dims),
                                                (C.c_int * max(n, 1))(*self._acts())))


class DSSM(KerasModule):
    """DSSM(user_feature_columns, item_feature_columns,
    user_dnn_hidden_units=(64, 32), item_dnn_hidden_units=(64, 32),
    dnn_activation='relu', dnn_use_bn=False, l2_reg_dnn=0, l2_reg_embedding=1e-6,
    dnn_dropout=0, loss_type='softmax', temperature=0.05, sampler_config=None,
    seed=1024) — model/dssm.py:17-90, forward only.

    ``forward(inputs)`` takes the dict gen_model_input builds (name -> array,
    utils/inputs.py:204-209) and returns, for ``loss_type='softmax'``, the
    per-sample in-batch softmax loss [B, 1] (InBatchSoftmaxLayer over the two
    embeddings and the ids of ``sampler_config.item_name``), for ``'logistic'``
    sigmoid(u . v / temperature) [B, 1].  ``user_embedding(inputs)`` /
    ``item_embedding(inputs)`` are the reference's user_embedding_model /
    item_embedding_model outputs: the l2-normalised tower outputs.

    A tower's input row is [SparseFeat rows in column order | pooled var-len
    features | dense values]; a var-len column with a ``length_name`` is pooled
    over t < length, one without over id != 0 (the tables are built with
    mask_zero).  Each tower is ONE rs_dssm_tower_fwd launch — ids to the
    normalised embedding, the row and the activations in LDS — when
    rs_dssm_tower_ok takes it; ``forward_unfused`` (and a dnn_use_bn / 'dice'
    / 'prelu' / too-wide tower) composes rs_concat_pieces + rs_seq_pool_fwd,
    rs_mlp_fwd or DNN.forward, rs_l2_normalize_fwd, bit-identical where both
    run.  An empty ``item_dnn_hidden_units`` normalises the input row.

    One table per ``embedding_name`` over user and item columns together, a
    later var-len column replacing the entry (utils/inputs.py:33-43): the
    item's movie_id and the user's hist_movie_id share a table.

    Deviation: the reference's inner_product calls
    tf.reduce_sum without an axis, which collapses the whole batch to one
    scalar; 'logistic' here reduces over the last axis and returns [B, 1].
    l2 / dropout are training-only; training (Adam) is not built.

    Keras weight names (``keras_weights`` / ``set_keras_weights`` round-trip):
    ``sparse_emb_{embedding_name}/embeddings`` or, when a var-len column shares
    the name, ``sparse_seq_emb_{last such column}/embeddings``; ``dnn/…`` the
    user tower's DNN (kernel{i}, bias{i}, bn{i}/…), ``dnn_1/…`` the item
    tower's."""

    def __init__(self, user_feature_columns, item_feature_columns, user_dnn_hidden_units=(64, 32),
                 item_dnn_hidden_units=(64, 32), dnn_activation="relu", dnn_use_bn=False, l2_reg_dnn=0,
                 l2_reg_embedding=1e-6, dnn_dropout=0, loss_type="softmax", temperature=0.05, sampler_config=None,
                 seed=1024, device=None):
        super().__init__(device, seed)
        if loss_type not in ("logistic", "softmax"):
            raise ValueError(" `loss_type` must be `logistic` or `softmax` ")
        ucols, icols = list(user_feature_columns), list(item_feature_columns)
        self.loss_type, self.temperature = loss_type, float(temperature)
        self.l2_reg_embedding = l2_reg_embedding
        for c in ucols + icols:
            if not isinstance(c, DenseFeat) and (c.use_hash or getattr(c, "weight_name", None) is not None):
                raise NotImplementedError(f"DSSM: column {c.name!r}: use_hash / weight_name are not built")
        # one table per embedding_name; a later var-len column replaces the entry (utils/inputs.py:33-43)
        spec = {}
        for c in ucols + icols:
            if isinstance(c, SparseFeat):
                spec[c.embedding_name] = (f"sparse_emb_{c.embedding_name}", c)
        for c in ucols + icols:
            if isinstance(c, VarLenSparseFeat):
                spec[c.embedding_name] = (f"sparse_seq_emb_{c.name}", c)
        self._table_names = {en: kn for en, (kn, _) in spec.items()}
        self.tables = torch.nn.ParameterDict()
        for en, (kn, c) in spec.items():
            shape = (int(c.vocabulary_size), int(c.embedding_dim))
            init = c.embeddings_initializer
            w = torch.randn(*shape, generator=self._gen).mul_(1e-4) if init is None else \
                torch.as_tensor(init(shape, self._gen), dtype=torch.float32).reshape(shape)
            self.tables[en] = torch.nn.Parameter(w.to(self._dev), requires_grad=False)
        for c in ucols + icols:
            if not isinstance(c, DenseFeat) and tuple(self.tables[c.embedding_name].shape) != \
                    (int(c.vocabulary_size), int(c.embedding_dim)):
                raise ValueError(f"DSSM: column {c.name!r} does not match the table of {c.embedding_name!r}")
        self.user_tower = _Tower(ucols, user_dnn_hidden_units, dnn_activation, l2_reg_dnn, dnn_dropout, dnn_use_bn,
                                 device, _subseed(self._gen))
        self.item_tower = _Tower(icols, item_dnn_hidden_units, dnn_activation, l2_reg_dnn, dnn_dropout, dnn_use_bn,
                                 device, _subseed(self._gen))
        if self.user_tower.out_width != self.item_tower.out_width:
            raise ValueError(f"DSSM: the towers' output widths differ ({self.user_tower.out_width} and "
                             f"{self.item_tower.out_width})")
        self.sampler_config, self.softmax = sampler_config, None
        if loss_type == "softmax":
            if sampler_config is None:
                raise ValueError("DSSM: loss_type 'softmax' needs a sampler_config (NegativeSampler)")
            if sampler_config.item_name not in self.item_tower.features:
                raise ValueError(f"DSSM: sampler_config.item_name {sampler_config.item_name!r} is not an item feature")
            self.softmax = InBatchSoftmaxLayer(sampler_config._asdict(), temperature, device=device)

    # ---- weights
    def keras_weights(self):
        out = {f"{self._table_names[en]}/embeddings": t for en, t in self.tables.items()}
        for prefix, tw in (("dnn", self.user_tower), ("dnn_1", self.item_tower)):
            if tw.dnn.layers:
                out.update({f"{prefix}/{k}": v for k, v in tw.dnn.keras_weights().items()})
        return out

    def set_keras_weights(self, weights, strict=True):
        own = self.keras_weights()
        if strict and set(own) != set(weights):
            raise KeyError(f"DSSM: missing {sorted(set(own) - set(weights))}, unknown {sorted(set(weights) - set(own))}")
        with torch.no_grad():
            for name, p in own.items():
                if name in weights:
                    p.copy_(torch.as_tensor(weights[name], dtype=torch.float32).reshape(p.shape))
        self._weights_changed()

    # ---- inputs
    def _pieces(self, tw, inputs):
        """(single-id / dense pieces [(width, column, source, table or None)],
        sequence features (seq_pool_arrays' tuples), batch)."""
        dev = self._dev
        pieces, seqs, B = [], [], None
        for c, at in zip(tw.sparse_cols, tw.sparse_at):
            ids = _ids_tensor(inputs[c.name], dev).reshape(-1).contiguous()
            pieces.append((c.embedding_dim, at, ids, self.tables[c.embedding_name]))
        for c, at in zip(tw.dense_cols, tw.dense_at):
            v = _to_device_f32(inputs[c.name], dev)
            pieces.append((c.dimension, at, v.reshape(v.shape[0], c.dimension), None))
        for c, at in zip(tw.varlen_cols, tw.varlen_at):
            ids = _ids_tensor(inputs[c.name], dev)
            if ids.dim() != 2 or ids.shape[1] != c.maxlen:
                raise ValueError(f"DSSM: {c.name!r} has shape {tuple(ids.shape)}, expected [batch, {c.maxlen}]")
            ids = ids.contiguous()
            L = None if c.length_name is None else _lengths(inputs[c.length_name], dev, ids.shape[0])
            seqs.append((c.embedding_dim, at, c.maxlen, c.combiner, ids, self.tables[c.embedding_name], L, None))
        for t in [p[2] for p in pieces] + [s[4] for s in seqs]:
            if B is not None and t.shape[0] != B:
                raise ValueError(f"DSSM: the inputs hold {B} and {t.shape[0]} samples")
            B = t.shape[0]
        return pieces, seqs, B

    @staticmethod
    def _piece_arrays(ch):
        n = len(ch)
        return (n, (C.c_int * n)(*[p[0] for p in ch]), (C.c_int * n)(*[p[1] for p in ch]),
                (C.c_int * n)(*[-1 if p[3] is None else _lib.id_kind(p[2]) for p in ch]),
                (C.c_void_p * n)(*[ptr(p[2]) for p in ch]),
                (C.c_int64 * n)(*[p[2].stride(0) if p[3] is None else 1 for p in ch]),
                (C.c_void_p * n)(*[ptr(p[3]) for p in ch]),
                (C.c_int64 * n)(*[0 if p[3] is None else p[3].shape[0] for p in ch]))

    def _tower_input(self, tw, pieces, seqs, B, err):
        """The tower's input row in HBM [B, input_width]: rs_concat_pieces + rs_seq_pool_fwd."""
        x = torch.empty(B, tw.input_width, dtype=torch.float32, device=self._dev)
        for i in range(0, len(pieces) if B else 0, _CC_MAXP):
            call("rs_concat_pieces", *self._piece_arrays(pieces[i:i + _CC_MAXP]), ptr(x), x.stride(0), B, ptr(err.t),
                 _lib.stream())
        seq_pool(seqs, x, B, err)
        return x

    def _embedding(self, tw, inputs, fused, check_ids):
        pieces, seqs, B = self._pieces(tw, inputs)
        err = _ErrFlag(self._dev)
        out = torch.empty(B, tw.out_width, dtype=torch.float32, device=self._dev)
        if fused and tw.fused_ok():
            if B:
                n = len(tw.dnn.layers)
                dims = [tw.input_width] + tw.dnn.hidden_units
                none = (None,) * 7
                pa = self._piece_arrays(pieces) if pieces else (0,) + none
                sa = (len(seqs),) + (seq_pool_arrays(seqs) if seqs else (None,) * 12)
                call("rs_dssm_tower_fwd", *pa, *sa, n, (C.c_int * (n + 1))(*dims), (C.c_int * max(n, 1))(*tw._acts()),
                     ptr(tw.prepared()) if n else None, ptr(out), out.stride(0), B, ptr(err.t), _lib.stream())
        else:
            x = self._tower_input(tw, pieces, seqs, B, err)
            if B:
                y = x if not tw.dnn.layers else (tw.tower(x) if tw.mlp_ok() else tw.dnn(x))
                l2_normalize(y, out=out)
        if check_ids:
            err.check("DSSM")
        return out

    def user_embedding(self, inputs, check_ids=True, fused=True):
        return self._embedding(self.user_tower, inputs, fused, check_ids)

    def item_embedding(self, inputs, check_ids=True, fused=True):
        return self._embedding(self.item_tower, inputs, fused, check_ids)

    def _forward(self, inputs, check_ids, fused):
        u = self._embedding(self.user_tower, inputs, fused, check_ids)
        v = self._embedding(self.item_tower, inputs, fused, check_ids)
        if self.loss_type == "softmax":
            return self.softmax([u, v, inputs[self.sampler_config.item_name]], check_ids=check_ids)
        B, E = u.shape
        out = torch.empty(B, 1, dtype=torch.float32, device=self._dev)
        # PredictionLayer('binary', use_bias=False) of the score: the sigmoid inside the launch
        call("rs_dssm_score_fwd", ptr(u), u.stride(0), ptr(v), v.stride(0), self.temperature, ptr(out), B, E,
             _lib.stream())
        return out

    def forward(self, inputs, check_ids=True):
        return self._forward(inputs, check_ids, True)

    def forward_unfused(self, inputs, check_ids=True):
        """The same forward from the stand-alone entries: rs_concat_pieces +
        rs_seq_pool_fwd into a [B, width] buffer, rs_mlp_fwd (DNN.forward for a
        tower it does not take), rs_l2_normalize_fwd."""
        return self._forward(inputs, check_ids, False)
