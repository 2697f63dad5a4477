"""DSSM — the reference's two-tower retrieval model (model/dssm.py:17-90),
forward and training step.  ``models.DSSM`` is this class."""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib, _train_ops
from ._lib import call, ints, ptr, ptrs
from ._train_ops import _dropout_rng, _subseed, bce_head_logit, bn_train_bwd, bn_train_fwd, gemm_ws, scratch
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
        return bool(_lib.lib().rs_dssm_tower_ok(n_pc + n_seq, n, ints(dims), ints(self._acts())))


class DSSM(KerasModule):
    """DSSM(user_feature_columns, item_feature_columns,
    user_dnn_hidden_units=(64, 32), item_dnn_hidden_units=(64, 32),
    dnn_activation='relu', dnn_use_bn=False, l2_reg_dnn=0, l2_reg_embedding=1e-6,
    dnn_dropout=0, loss_type='softmax', temperature=0.05, sampler_config=None,
    seed=1024) — model/dssm.py:17-90, forward and one step of its Keras fit
    (``gradients`` / ``train_step`` / ``fit``: Adam on the batch mean of the
    in-batch softmax losses, model/dssm.py:149-152).

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
    l2 / dropout are training-only (``train_step``).

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
        return (n, ints([p[0] for p in ch]), ints([p[1] for p in ch]),
                ints([-1 if p[3] is None else _lib.id_kind(p[2]) for p in ch]), ptrs([p[2] for p in ch]),
                (C.c_int64 * n)(*[p[2].stride(0) if p[3] is None else 1 for p in ch]), ptrs([p[3] for p in ch]),
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
                call("rs_dssm_tower_fwd", *pa, *sa, n, ints(dims), ints(tw._acts()),
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

    # ---- retrieval
    def _predict(self, tw, inputs, batch_size, check_ids, fused):
        batch_size = int(batch_size)
        if batch_size < 1:
            raise ValueError("DSSM: batch_size must be at least 1")
        n = len(inputs[(tw.sparse_cols + tw.varlen_cols + tw.dense_cols)[0].name])
        if n == 0:
            return torch.empty(0, tw.out_width, dtype=torch.float32, device=self._dev)
        return torch.cat([self._embedding(tw, {k: v[i:i + batch_size] for k, v in inputs.items()}, fused, check_ids)
                          for i in range(0, n, batch_size)])

    def predict_user_embedding(self, inputs, batch_size=4096, check_ids=True, fused=True):
        """The reference's user_embedding_model.predict(inputs, batch_size=2**12)
        (model/dssm.py:154-160): ``user_embedding`` over sequential batches of
        ``batch_size`` rows (the last one short), concatenated [rows, E]."""
        return self._predict(self.user_tower, inputs, batch_size, check_ids, fused)

    def predict_item_embedding(self, inputs, batch_size=4096, check_ids=True, fused=True):
        """item_embedding_model.predict: ``item_embedding`` over batches, concatenated."""
        return self._predict(self.item_tower, inputs, batch_size, check_ids, fused)

    def retrieve(self, user_inputs, item_inputs, N=50, batch_size=4096, fused=None, item_ids=None):
        """(item_ids int64 [U, N], score float32 [U, N]): for every user the N
        items with the largest u . v, best first (a tie goes to the item that
        comes first in ``item_inputs``); padded with (-1, -inf) where there are
        fewer than N items.  ``user_inputs`` / ``item_inputs``: the towers'
        input dicts (embedded in batches of ``batch_size``), or an embedding
        matrix computed before (``predict_*_embedding``).  The ids are
        ``item_ids`` if given, else ``item_inputs[sampler_config.item_name]``,
        else (no sampler_config, or a precomputed item matrix) the positions.
        ``fused``: retrieval.topn_inner_product's — None / True the
        rs_topn_inner_product kernel, False the torch composition."""
        from .retrieval import topn_inner_product
        is_matrix = lambda x: not isinstance(x, dict)  # noqa: E731
        u = _to_device_f32(user_inputs, self._dev) if is_matrix(user_inputs) else \
            self.predict_user_embedding(user_inputs, batch_size)
        v = _to_device_f32(item_inputs, self._dev) if is_matrix(item_inputs) else \
            self.predict_item_embedding(item_inputs, batch_size)
        if item_ids is None and not is_matrix(item_inputs) and self.sampler_config is not None:
            item_ids = item_inputs[self.sampler_config.item_name]
        pos, score = topn_inner_product(u, v, N, fused=fused)
        pos = pos.to(torch.int64)
        if item_ids is None:
            return pos, score
        ids = torch.as_tensor(item_ids).to(self._dev).reshape(-1).to(torch.int64)
        if ids.numel() != v.shape[0]:
            raise ValueError(f"DSSM.retrieve: {ids.numel()} item ids for {v.shape[0]} items")
        if ids.numel() == 0:
            return pos, score
        return torch.where(pos < 0, pos, ids[pos.clamp(min=0)]), score

    def recall(self, user_inputs, true_items, item_inputs, N=50, batch_size=4096, fused=None, item_ids=None):
        """The mean over the users of ``recall_N([true item], retrieved ids, N)``
        (utils/negative.py:53-54 with one true item per user): the share of users
        whose true item is among their N retrieved.  The hit test runs on the
        device; one number comes back."""
        ids, _ = self.retrieve(user_inputs, item_inputs, N, batch_size, fused, item_ids)
        t = torch.as_tensor(true_items).to(self._dev).reshape(-1).to(torch.int64)
        if t.numel() != ids.shape[0]:
            raise ValueError(f"DSSM.recall: {t.numel()} true items for {ids.shape[0]} users")
        if t.numel() == 0:
            raise ValueError("DSSM.recall: no users")
        return float((ids == t.unsqueeze(1)).any(1).to(torch.float32).mean())

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

    # ---- training
    _TRAIN_ACTS = (None, "linear", "relu", "sigmoid")

    def _check_train(self, labels):
        for tw in (self.user_tower, self.item_tower):
            if any(l.activation not in self._TRAIN_ACTS for l in tw.dnn.layers):
                raise NotImplementedError("DSSM: training takes 'relu' / 'sigmoid' / linear tower layers only")
        if self.loss_type == "logistic" and labels is None:
            raise ValueError("DSSM: loss_type 'logistic' needs labels to train")

    def _tower_train_fwd(self, tw, x, dt, drop, st):
        """DNN(..., output_activation='linear') in training mode on x [B, width]:
        Dense, BatchNormalization on the batch's statistics, the activation,
        the Dropout draw (layer/core.py:187-205).  Returns what _tower_train_bwd
        reads; ctx["out"] is the tower's output."""
        dnn, B = tw.dnn, x.shape[0]
        ctx = {"in": [x], "pre": [], "bn": [], "saved": [], "act": [], "offs": []}
        for i, l in enumerate(dnn.layers):
            z = dt.dense(ctx["in"][-1], l, B)
            bn_saved = None
            if dnn.use_bn:
                ctx["bn"].append(z)
                bn_saved, z = bn_train_fwd(dnn.bn_layers[i], z, st)
            saved, y = (None, z) if l.activation in (None, "linear") else dt.act_fwd(l, z, B)
            ctx["pre"].append(z), ctx["saved"].append((bn_saved, saved)), ctx["act"].append(y)
            if drop is not None:
                y = y.clone()  # (the activation's backward reads its undropped output)
                ctx["offs"].append(drop[0].draw(y, drop[1], st))
            ctx["in"].append(y)
        ctx["out"] = ctx["in"][-1]
        return ctx

    def _tower_train_bwd(self, tw, ctx, dh, dt, drop, st):
        """dL/d(input row) from dh = dL/d(tower output); the layers' gradients go to dt.updates."""
        dnn, B = tw.dnn, dh.shape[0]
        for i in reversed(range(len(dnn.layers))):
            l = dnn.layers[i]
            if drop is not None:  # the forward's mask, regenerated from its offset
                dh = dh.contiguous()
                drop[0].redraw(dh, drop[1], ctx["offs"][i], st)
            dz = dh if l.activation in (None, "linear") else \
                dt.act_bwd(l, ctx["pre"][i], ctx["act"][i], ctx["saved"][i][1], dh, B)
            if dnn.use_bn:
                bn = dnn.bn_layers[i]
                dz, dgam, dbet = bn_train_bwd(bn, ctx["bn"][i], ctx["saved"][i][0], dz.contiguous(), st)
                dt.updates.extend([(bn.gamma, dgam, 0.0), (bn.beta, dbet, 0.0)])
            dh = dt.dense_bwd(l, ctx["in"][i], dz, l2=float(dnn.l2_reg or 0))
        return dh

    def _grad_accum(self, G, ids, T, lengths, combiner, grad_ptr, grad_stride, B, err, st):
        """rs_embedding_grad_accum of one id source into the dense table gradient G."""
        ws = scratch(self, "_ega_ws", _lib.lib().rs_embedding_grad_accum_workspace_size(B * T))
        call("rs_embedding_grad_accum", ptr(G), G.shape[0], G.shape[1], ptr(ids), _lib.id_kind(ids),
             ids.stride(0) if ids.dim() == 2 else 1, T, ptr(lengths), 0 if lengths is None else _lib.id_kind(lengths),
             combiner, grad_ptr, grad_stride, B, ptr(ws), ptr(err.t), st)

    def _table_grads(self, sources, B, err, st):
        """One zero-fill per table, then one rs_embedding_grad_accum per id
        source in a fixed order: user columns, then item columns, each in
        input-row order.  A 'max' column (its gradient goes to the positions
        that hold the maximum, a tie split evenly as TF's reduce_max does) is
        composed in torch and added through the same entry."""
        name_of = {id(t): en for en, t in self.tables.items()}
        G = self.__dict__.setdefault("_table_grad_bufs", {})
        for en, t in self.tables.items():
            if en not in G or G[en].shape != t.shape:
                G[en] = torch.empty_like(t)
            G[en].zero_()
        for (pieces, seqs), dx in sources:
            for width, at, ids, table in pieces:
                if table is not None:
                    self._grad_accum(G[name_of[id(table)]], ids, 1, None, -1, dx.data_ptr() + 4 * at, dx.stride(0), B,
                                     err, st)
            for E, at, T, comb, ids, table, L, _ in seqs:
                g = G[name_of[id(table)]]
                if comb != "max":
                    self._grad_accum(g, ids, T, L, {"sum": 0, "mean": 1}[comb], dx.data_ptr() + 4 * at, dx.stride(0), B, err,
                                     st)
                    continue
                valid = (torch.arange(T, device=self._dev).unsqueeze(0) < L.unsqueeze(1)) if L is not None \
                    else ids.ne(0)
                rows = table[ids.long().clamp(0, table.shape[0] - 1)] - (~valid).unsqueeze(-1) * 1e9
                tie = (rows == rows.max(1, keepdim=True).values).to(torch.float32)
                gr = (tie / tie.sum(1, keepdim=True) * dx[:, at:at + E].unsqueeze(1)).reshape(B * T, E).contiguous()
                self._grad_accum(g, ids.reshape(B * T), 1, None, -1, gr.data_ptr(), E, B * T, err, st)
        return G

    def gradients(self, inputs, labels=None, check_ids=True, dropout=None):
        """(grads, losses) of one training batch: ``grads`` maps the Keras name
        of every trainable weight (``keras_weights()`` without the moving
        statistics) to the gradient of the DATA loss — the batch mean of the
        per-sample losses; tables dense [vocab, E] with exact zeros in rows
        nobody looked up; no regulariser — and ``losses`` is the per-sample
        [B, 1] before the step (the in-batch softmax loss, or the BCE of
        sigmoid(u . v / temperature) against ``labels`` for 'logistic').  No
        weight changes except BatchNormalization's moving statistics.
        The table gradients live in buffers the model keeps: they hold until
        the next call.

        Order: the tower inputs (rs_concat_pieces + rs_seq_pool_fwd) and the
        id check; each tower in training mode (rs_dense_fwd, rs_bn_train_fwd,
        the dropout draws, as DIEN's tower); rs_l2_normalize_fwd,
        rs_inbatch_softmax_train_fwd, rs_inbatch_softmax_bwd (an embedding
        wider than rs_inbatch_softmax_bwd_ok: the same math in torch ops),
        rs_l2_normalize_bwd; the towers backward; rs_embedding_grad_accum per
        id source.  ``dropout``: None applies dnn_dropout, False turns it off,
        a float overrides the rate."""
        self._check_train(labels)
        dev, st = self._dev, _lib.stream()
        towers = (self.user_tower, self.item_tower)
        rate = [0.0 if dropout is False else float(tw.dnn.dropout_rate or 0) if dropout is None or dropout is True
                else float(dropout) for tw in towers]
        # ---- inputs: every id is checked before anything else is touched
        err = _ErrFlag(dev)
        src = [self._pieces(tw, inputs) for tw in towers]
        B = src[0][2]
        if src[1][2] != B:
            raise ValueError(f"DSSM: the inputs hold {B} and {src[1][2]} samples")
        if not B:
            raise ValueError("DSSM: an empty batch")
        xs = [self._tower_input(tw, p, s, B, err) for tw, (p, s, _) in zip(towers, src)]
        idx = None
        if self.loss_type == "softmax":
            idx = torch.as_tensor(inputs[self.sampler_config.item_name])
            if idx.dtype not in (torch.int32, torch.int64):
                idx = idx.to(torch.int64)
            idx = idx.to(dev).reshape(-1).contiguous()
            if check_ids and bool(((idx < 0) | (idx >= self.softmax.logq.numel())).any()):
                raise _lib.BadIdError("DSSM: item index out of range of sampler_config.item_count")
        if check_ids:
            err.check("DSSM")
        shapes = [(l.kernel.shape[0], l.kernel.shape[1], B) for tw in towers for l in tw.dnn.layers] or [(1, 1, B)]
        dt = _train_ops.DenseTrain(gemm_ws(self, _train_ops.dense_train_need(shapes)), st, dev)
        emp = dt.emp

        # ---- forward
        drops = [(_dropout_rng(self), r, None) if r > 0 else None for r in rate]
        ctx = [self._tower_train_fwd(tw, x, dt, d, st) for tw, x, d in zip(towers, xs, drops)]
        yu, yv = (c["out"].contiguous() for c in ctx)
        u, v = l2_normalize(yu), l2_normalize(yv)
        E = u.shape[1]
        if self.loss_type == "softmax":
            logq, temp = self.softmax.logq, self.temperature
            if _lib.lib().rs_inbatch_softmax_bwd_ok(E):
                losses, lse, du, dv = emp(B, 1), emp(B), emp(B, E), emp(B, E)
                head = (ptr(u), E, ptr(v), E, ptr(idx), _lib.id_kind(idx), ptr(logq), logq.numel(), temp)
                call("rs_inbatch_softmax_train_fwd", *head, ptr(losses), ptr(lse), B, E, ptr(err.t), st)
                call("rs_inbatch_softmax_bwd", *head, ptr(lse), None, ptr(du), E, ptr(dv), E, B, E, ptr(err.t), st)
            else:
                z = (u / temp) @ v.t() - logq[idx.long()].unsqueeze(0)
                lse = torch.logsumexp(z, dim=1)
                losses = (lse - torch.diagonal(z)).unsqueeze(1)
                dz = (torch.exp(z - lse.unsqueeze(1)) - torch.eye(B, device=dev)) / B
                du, dv = (dz @ v) / temp, dz.t() @ (u / temp)
        else:
            t = _to_device_f32(labels, dev).reshape(-1)
            if t.numel() != B:
                raise ValueError(f"DSSM: {t.numel()} labels for a batch of {B}")
            g, loss = bce_head_logit(((u * v).sum(1) / self.temperature).contiguous(), t, True, st)
            losses = loss.unsqueeze(1)
            du, dv = g.unsqueeze(1) * v / self.temperature, g.unsqueeze(1) * u / self.temperature
            du, dv = du.contiguous(), dv.contiguous()

        # ---- backward
        dxs = []
        for tw, c, y, d, drop in zip(towers, ctx, (yu, yv), (du, dv), drops):
            call("rs_l2_normalize_bwd", ptr(y), y.stride(0), ptr(d), d.stride(0), ptr(d), d.stride(0), B, E, st)
            dxs.append(self._tower_train_bwd(tw, c, d, dt, drop, st).contiguous())
        if any(d is not None for d in drops):
            _dropout_rng(self).end_step(st)
        G = self._table_grads([((p, s), dx) for (p, s, _), dx in zip(src, dxs)], B, err, st)
        by_param = {id(w): g for w, g, _ in dt.updates}
        grads = {}
        for name, p in self.keras_weights().items():
            if name.endswith("/embeddings"):
                en = next(e for e, kn in self._table_names.items() if f"{kn}/embeddings" == name)
                grads[name] = G[en]
            elif id(p) in by_param:
                grads[name] = by_param[id(p)]
        self._weights_changed()  # (the moving statistics moved)
        return grads, losses

    def _l2_of(self, name):
        if name.endswith("/embeddings"):
            return float(self.l2_reg_embedding or 0)
        if name.rsplit("/", 1)[-1].startswith("kernel"):
            tw = self.item_tower if name.startswith("dnn_1/") else self.user_tower
            return float(tw.dnn.l2_reg or 0)
        return 0.0

    def optimizer(self, lr=0.001):
        """The model's Adam (optim.Adam), created on first use."""
        opt = self.__dict__.get("_adam")
        if opt is None:
            from .optim import Adam
            opt = self.__dict__["_adam"] = Adam(lr=lr, device=self._dev)
        return opt

    def train_step(self, inputs, labels=None, lr=0.001, return_loss=False, check_ids=True, dropout=None):
        """One step of Keras fit (model/dssm.py:149-152: Adam, lr 0.001, on the
        batch mean of the per-sample losses): exactly ``gradients`` followed by
        one ``Adam.apply`` over every trainable weight, with l2_reg_embedding
        on the whole tables and l2_reg_dnn on the tower kernels folded into
        the optimizer entry (gradient + 2 l2 w).  Adam is applied to every row
        of every table each step, as Keras does: the tables' regulariser makes
        their gradient dense, and Keras' non-lazy sparse Adam decays the moments
        of untouched rows even without it.  Every id is checked before any
        weight changes.  A 'max'-pooled column raises NotImplementedError.
        Returns the per-sample losses [B, 1] before the step when
        ``return_loss``."""
        for tw in (self.user_tower, self.item_tower):
            if any(c.combiner == "max" for c in tw.varlen_cols):
                raise NotImplementedError("DSSM.train_step: 'max' pooling is not built (sum / mean only)")
        self._check_train(labels)
        opt = self.optimizer(lr)
        grads, losses = self.gradients(inputs, labels, check_ids=check_ids, dropout=dropout)
        own = self.keras_weights()
        opt.apply([(own[name], g, self._l2_of(name)) for name, g in grads.items()], _lib.stream(), lr=lr)
        self._weights_changed()
        return losses if return_loss else None

    def fit(self, inputs, labels=None, batch_size=256, epochs=1, lr=0.001):
        """``train_step`` over sequential batches of ``batch_size`` (the last
        one short), ``epochs`` times; returns the mean per-sample loss of each
        epoch.  Deviation: Keras' fit shuffles the samples every epoch, this
        keeps their order."""
        n, batch_size = len(next(iter(inputs.values()))), int(batch_size)
        history = []
        for _ in range(int(epochs)):
            total = torch.zeros((), dtype=torch.float64, device=self._dev)
            for i in range(0, n, batch_size):
                xb = {k: v[i:i + batch_size] for k, v in inputs.items()}
                lb = None if labels is None else labels[i:i + batch_size]
                total += self.train_step(xb, lb, lr=lr, return_loss=True).sum(dtype=torch.float64)
            history.append(float(total) / n)
        return history
