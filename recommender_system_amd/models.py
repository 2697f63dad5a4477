"""Keras-Model-compatible CTR models on the MI355X kernels.

Same names, constructor arguments and forward semantics as the reference's
models (Hcyand/recommender_system, algorithm/deep_learning/model/):

  FM(k, w_reg=1e-4, v_reg=1e-4)                                   model/fm.py:14-23
  DeepFM(feature_columns, k, w_reg, v_reg, hidden_units, output_dim, activation)
                                                                  model/deepFM.py:15-31
  DCN(feature_columns, hidden_units, output_dim, activation, layer_num, reg_w, reg_b)
                                                                  model/dcn.py:15-34
  PNN(feature_columns, mode, hidden_units, output_dim, activation='relu',
      dropout=0.2, use_fgcnn=False)                               model/pnn.py:14-53
  DIN(feature_columns, behavior_feature_list, att_hidden_units=(80, 40),
      dnn_hidden_units=(256, 128, 64), att_attention='prelu',
      dnn_activation='prelu', dnn_dropout=0.0)                    model/din.py:15-95
  NFM(feature_columns, hidden_units, output_dim, activation='relu', dropout=0)
                                                                  model/nfm.py:13-33
  AFM(feature_columns, mode)                                      model/afm.py:11-19
  FFM(feature_columns, k, w_reg=1e-4, v_reg=1e-4)                 model/ffm.py:10-22
  DeepCrossing(feature_columns, k, hidden_units, res_layer_num)   model/deepCrossing.py:15-32
  WideDeep(feature_columns, hidden_units, output_dim, activation) model/wideDeep.py:14-34
  FNN(k, hidden_units, output_dim=1, activation='relu', w_reg, v_reg)  model/fnn.py:13-67
  MMOE(mmoe_hidden_units, num_experts, num_tasks, tower_hidden_units, output_dim,
       activation='relu', use_expert_bias=True, use_gate_bias=True) model/mmoe.py:10-32
  DIEN(dnn_feature_columns, history_feature_list, gru_type='GRU', ...)
                                                                  model/dien.py:83-169
  DSSM(user_feature_columns, item_feature_columns, ...)           model/dssm.py:17-90 (dssm.py)

Criteo-style models take the reference's packed input X[B, 13+F] (dense
features followed by label-encoded sparse ids, as floats — Keras casts them to
int32 inside Embedding, so ids are exact only below 2**24), or the pair
``(dense[B,13] float, ids[B,F] int32/int64)`` which lifts that limit.

Extra keyword ``embed_dim`` (default 8, the reference's EmbedLayer default)
sets the embedding width: the reference ignores feat['embed_dim'] and always
uses k=8 (layer/core.py:268-271), so 8 is the drop-in behaviour.

PNN runs with 3-D embeddings [B,F,k] (documented deviation: the reference's
rank-2 EmbedLayer makes PNN.call raise at model/pnn.py:38).  Modes 'inner',
'outer' and 'both' are built (forward and training); an unknown mode raises
the reference's ValueError.  use_fgcnn=True (HIP device only: building it for
another device raises NotImplementedError; trained only when built with
``train_fgcnn=True``, see PNN) runs the product
layers and the flat part on z = concat([embed, FGCNNLayer(embed)], axis=1)
(model/pnn.py:33-48); extra keyword ``fgcnn`` passes FGCNNLayer's arguments.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib, _train_ops
from ._lib import call, ints, ptr, ptrs, sized
from .layers import (AFMLayer, Attention, BatchNormalization, CrossLayer, Dense, DNNLayer, EmbedLayer, FFMLayer,
                     FGCNNLayer, FMLayer, InnerProductLayer, OuterProductLayer,
                     KerasModule, ResLayer, TowerMixin, WideLayer, sigmoid_combine, _ids_tensor, _to_device_f32,
                     _AFM_MODES, _ErrFlag, _RES_MAXH, _RES_MAXU, _res_params, _res_ok, _res_prepare, mmoe_layer,
                     tower_layer, _MMOE_MAXL, _mmoe_dims, _mmoe_input, _mmoe_ok, _mmoe_params, _mmoe_prepare,
                     DNN, InterestEvolution, PredictionLayer, _glorot_normal)
from .feature_column import DenseFeat, SparseFeat, VarLenSparseFeat, build_input_features


from ._train_ops import (_Dropout, _check_train_tower, _dnn_apply, _dnn_backward, _dnn_train_forward,  # noqa: F401
                         _dnn_updates, _dropout_rate, _dropout_rng, _split_criteo, _subseed, bce_head,
                         bce_head_logit, bn_train_bwd, bn_train_fwd, dense_backward, embedding_sgd,
                         embedding_sgd_strided, fm_backward, fm_xv, gemm_need, gemm_ws, scratch,
                         MMOE_L2, mmoe_head, mmoe_labels, mmoe_layer_grads)


class FM(KerasModule):
    """FM(k, w_reg, v_reg) — model/fm.py:14-23: sigmoid(FMLayer(x)).

    ``forward(x[B,n])`` takes the reference's one-hot matrix (any dense x).
    ``forward_onehot(dense, ids, field_offsets)`` takes its compact form and
    gathers rows of v/w1 instead of multiplying by zeros (same result: the
    one-hot block has exactly one 1 per field, utils/dataset.py:47-48)."""

    def __init__(self, k, w_reg=1e-4, v_reg=1e-4, device=None, seed=None, print_shape=False):
        super().__init__(device, seed)
        self.fm = FMLayer(k, w_reg, v_reg, device=device, seed=_subseed(self._gen))
        self.print_shape = print_shape  # the reference prints inputs.shape (model/fm.py:20)

    def forward(self, inputs):
        if self.print_shape:
            print(tuple(inputs.shape))
        logit = self.fm(inputs)
        return sigmoid_combine(logit)

    def forward_onehot(self, dense, ids, field_offsets, field_vocab, check_ids=True):
        dense = _to_device_f32(dense, self._dev)
        ids = _ids_tensor(ids, self._dev)
        offs = torch.as_tensor(field_offsets, dtype=torch.int64, device=self._dev)
        voc = torch.as_tensor(field_vocab, dtype=torch.int64, device=self._dev)
        B, nd = dense.shape
        n = nd + int(voc.sum())
        if not self.fm.built:
            self.fm.build(n)
        logit = torch.empty(B, 1, dtype=torch.float32, device=self._dev)
        err = _ErrFlag(self._dev)
        call("rs_fm_onehot_fwd", ptr(ids), _lib.id_kind(ids), ids.stride(0), ptr(dense), dense.stride(0), nd,
             ptr(offs), ptr(voc), ids.shape[1], ptr(self.fm.w1), ptr(self.fm.w0), ptr(self.fm.v), self.fm.k,
             ptr(logit), B, ptr(err.t), _lib.stream())
        if check_ids:
            err.check("FM")
        return sigmoid_combine(logit)

    def train_step(self, dense, ids, labels, field_offsets, field_vocab, lr=0.01, return_loss=False,
                   check_ids=True):
        """One step of compile_fit (utils/compile_fit.py:9-15: SGD(lr),
        binary cross-entropy, FMLayer's l2 regularisers) on a compact batch
        (dense [B,nd], label codes [B,F] of the one-hot x): one
        rs_fm_train_step call updates w0 / w1 / v in place.  Returns the
        per-sample losses before the step if ``return_loss``."""
        dense = _to_device_f32(dense, self._dev)
        ids = _ids_tensor(ids, self._dev)
        labels = _to_device_f32(labels, self._dev).reshape(-1)
        offs = torch.as_tensor(field_offsets, dtype=torch.int64, device=self._dev)
        voc = torch.as_tensor(field_vocab, dtype=torch.int64, device=self._dev)
        B, nd = dense.shape
        F = ids.shape[1]
        fm = self.fm
        if not fm.built:  # (a host sum: not inside a graph capture)
            fm.build(nd + int(voc.sum()))
        n = fm.w1.shape[0]
        ws = scratch(self, "_train_ws", _lib.lib().rs_fm_train_workspace_size(B, F, fm.k, nd))
        loss = torch.empty(B, dtype=torch.float32, device=self._dev) if return_loss else None
        err = _ErrFlag(self._dev)
        call("rs_fm_train_step", ptr(ids), _lib.id_kind(ids), ids.stride(0), ptr(dense), dense.stride(0), nd,
             ptr(offs), ptr(voc), F, fm.k, ptr(fm.w0), ptr(fm.w1), ptr(fm.v), n, ptr(labels), B, float(lr),
             float(fm.reg_w), float(fm.reg_b), ptr(ws), ptr(loss), ptr(err.t), _lib.stream())
        fm._invalidate()  # packed operand images of the old weights are stale
        if check_ids:
            err.check("FM.train_step")
        return loss


class DeepFM(KerasModule):
    """DeepFM — model/deepFM.py:15-31: x = [dense | EmbedLayer(sparse)],
    sigmoid(0.5*(FMLayer(x) + DNNLayer(x))).  Embedding lookup + concat + FM
    run as ONE fused kernel (rs_embed_fm_fwd) that also emits x for the DNN."""

    def __init__(self, feature_columns, k, w_reg, v_reg, hidden_units, output_dim, activation,
                 embed_dim=8, device=None, seed=None):
        super().__init__(device, seed)
        self.dense_feature_columns, self.sparse_feature_columns = feature_columns
        self.nd = len(self.dense_feature_columns)
        self.embed_layer = EmbedLayer(self.sparse_feature_columns, embed_dim, device=device, seed=_subseed(self._gen))
        d = self.nd + self.embed_layer.n_fields * embed_dim
        self.fm = FMLayer(k, w_reg, v_reg, device=device, seed=_subseed(self._gen), input_dim=d)
        self.dnn = DNNLayer(hidden_units, output_dim, activation, device=device, seed=_subseed(self._gen))
        self.dnn.build(d)
        self._err = _ErrFlag(self._dev)

    def fm_logit(self, inputs, x_out=None, check_ids=True):
        """The north-star hot path: ids -> rows -> FM logit in one launch."""
        dense, ids = _split_criteo(inputs, self.nd, self._dev)
        B = ids.shape[0]
        e = self.embed_layer
        prep = self.fm.prepared(self.nd, e.n_fields, e.k)
        logit = torch.empty(B, 1, dtype=torch.float32, device=self._dev)
        hoff, hvoc = e.host_meta()
        call("rs_embed_fm_fwd_hm", ptr(ids), _lib.id_kind(ids), ids.stride(0), ptr(dense), dense.stride(0), self.nd,
             ptr(e.table), ptr(e.field_offsets), ptr(e.field_vocab), hoff, hvoc, e.n_fields, e.k, ptr(prep),
             ptr(self.fm.w0), self.fm.k, ptr(logit), ptr(x_out), B, ptr(self._err.t), _lib.stream())
        if check_ids:
            self._err.check("DeepFM")
        return logit

    def fm_logit_stream(self, dense, ids, last_batch=None, min_blocks=1, out=None, check_ids=True):
        """The hot path over S consecutive batch requests in ONE launch
        (rs_embed_fm_fwd_hm_stream): dense [S, B, nd] f32, ids [S, B, F]
        int32 / int64 (contiguous per batch); the last batch may hold only
        ``last_batch`` samples.  Returns logits [S, B, 1] (rows past
        last_batch of the last batch untouched), each batch bit-identical to
        ``fm_logit`` on it alone."""
        S, B, F = ids.shape
        e = self.embed_layer
        if F != e.n_fields or dense.shape[:2] != (S, B) or dense.shape[2] != self.nd:
            raise ValueError("fm_logit_stream: dense [S, B, nd] and ids [S, B, F] expected")
        if ids.stride(2) != 1 or dense.stride(2) != 1:
            raise ValueError("fm_logit_stream: the last axis must be contiguous")
        prep = self.fm.prepared(self.nd, e.n_fields, e.k)
        logit = out if out is not None else torch.empty(S, B, 1, dtype=torch.float32, device=self._dev)
        hoff, hvoc = e.host_meta()
        call("rs_embed_fm_fwd_hm_stream", ptr(ids), _lib.id_kind(ids), ids.stride(1), ids.stride(0), ptr(dense),
             dense.stride(1), dense.stride(0), self.nd, ptr(e.table), hoff, hvoc, e.n_fields, e.k, ptr(prep),
             ptr(self.fm.w0), self.fm.k, ptr(logit), logit.stride(0), B, S, B if last_batch is None else last_batch,
             min_blocks, ptr(self._err.t), _lib.stream())
        if check_ids:
            self._err.check("DeepFM")
        return logit

    def train_step(self, inputs, labels, lr=0.01, return_loss=False, check_ids=True, dropout=None):
        """One step of compile_fit (utils/compile_fit.py:9-15: SGD(lr),
        binary cross-entropy on sigmoid(0.5 (FM + DNN)), FMLayer's l2
        regularisers) on a batch, every weight updated in place: the DNN's
        kernels/biases, w0 / w1 / v, and the looked-up embedding rows
        (row-sparse, duplicates summed in lookup order — rs_embedding_sgd).
        Forward with saved activations (rs_embed_gather, rs_dense_fwd,
        rs_fm_fwd), backward through rs_gemm / rs_col_sum / rs_fm_x_grad /
        rs_fm_param_grads, all gradients from the pre-step weights, then the
        updates.  Supports output_dim 1 and 'relu' / linear hidden layers.
        DNNLayer's Dropout runs in training mode as under Keras' fit (rate =
        the layer's, 0.2 by default; dropout=False turns it off): inverted
        dropout with counter-based masks (rs_dropout), the same masks in the
        backward."""
        dense, ids = _split_criteo(inputs, self.nd, self._dev)
        labels = _to_device_f32(labels, self._dev).reshape(-1)
        e, fm, dnn = self.embed_layer, self.fm, self.dnn
        layers = list(dnn.hidden_layer) + [dnn.output_layer]
        if dnn.output_layer.units != 1:
            raise NotImplementedError("DeepFM.train_step: output_dim 1 only")
        _check_train_tower("DeepFM", dnn)
        rate = _dropout_rate(dnn, dropout)
        B, dev, st = ids.shape[0], self._dev, _lib.stream()
        d, kfm = self.nd + e.n_fields * e.k, fm.k
        emp = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
        # forward, keeping what the backward needs
        x = e.gather(ids, dense, check_ids=check_ids)
        acts, drop = _dnn_train_forward(self, dnn, x, rate, st)
        dnn_out = dnn.output_layer(acts[-1])
        fm_out = fm(x)
        gw = gemm_ws(self, gemm_need([(*L.kernel.shape, B) for L in layers]))
        s = fm_xv(x, fm.v, gw, st)
        g_fm, g_dnn, loss = bce_head(fm_out, dnn_out, labels, 0.5, 0.5, return_loss, st)
        grads, delta = _dnn_backward(layers, acts, g_dnn.view(B, 1), gw, emp, st, drop=drop)
        dx = delta  # [B, d]: the DNN's gradient w.r.t. x; the FM's is added next
        dw1, dv, dw0 = fm_backward(x, s, fm.w1, fm.v, g_fm, dx, st)
        # updates (every gradient above used the pre-step weights)
        _lib.sgd_update_multi(_dnn_updates(grads) + [(fm.w1, dw1, d, fm.reg_w), (fm.v, dv, d * kfm, fm.reg_b),
                                                     (fm.w0, dw0, 1, 0.0)], lr, st)
        embedding_sgd(e, ids, ptr(dx) + 4 * self.nd, d, lr, st, self)
        self._weights_changed()  # packed operand images of the old weights are stale
        return loss

    def _fused_rows(self):
        """Tower input permutation for the fused kernel: its LDS tile holds
        [emb F*k | dense nd]; Keras rows are [dense nd | emb F*k]."""
        e = self.embed_layer
        fk = e.n_fields * e.k
        kp = (fk + self.nd + 15) // 16 * 16
        if getattr(self, "_in_rows", None) is None:
            rows = torch.full((kp,), -1, dtype=torch.int32)
            rows[:fk] = torch.arange(fk, dtype=torch.int32) + self.nd
            rows[fk:fk + self.nd] = torch.arange(self.nd, dtype=torch.int32)
            self._in_rows = rows.to(self._dev)
        return self._in_rows

    def fused_ok(self):
        e = self.embed_layer
        if not self.dnn.tower_ok():
            return False
        dims = self.dnn._dims()
        return bool(_lib.lib().rs_deepfm_fused_ok(self.nd, e.n_fields, e.k, self.fm.k, len(dims) - 1, ints(dims)))

    def forward_fused(self, inputs, check_ids=True, fm_logit=None):
        """DeepFM.call as ONE kernel (rs_deepfm_fwd)."""
        dense, ids = _split_criteo(inputs, self.nd, self._dev)
        B = ids.shape[0]
        e = self.embed_layer
        prep = self.fm.prepared(self.nd, e.n_fields, e.k)
        mlp = self.dnn.prepared(self._fused_rows())
        dims = self.dnn._dims()
        n = len(dims) - 1
        acts = [_lib.ACT[l.activation] for l in self.dnn._layers()]
        out = torch.empty(B, 1, dtype=torch.float32, device=self._dev)
        hoff, hvoc = e.host_meta()
        call("rs_deepfm_fwd_hm", ptr(ids), _lib.id_kind(ids), ids.stride(0), ptr(dense), dense.stride(0), self.nd,
             ptr(e.table), ptr(e.field_offsets), ptr(e.field_vocab), hoff, hvoc, e.n_fields, e.k, ptr(prep),
             ptr(self.fm.w0), self.fm.k, n, ints(dims), ints(acts), ptr(mlp), 0.5, 0.5,
             ptr(out), ptr(fm_logit), B, ptr(self._err.t), _lib.stream())
        if check_ids:
            self._err.check("DeepFM")
        return out

    def forward(self, inputs, check_ids=True):
        if self.fused_ok():
            return self.forward_fused(inputs, check_ids)
        return self.forward_unfused(inputs, check_ids)

    def forward_unfused(self, inputs, check_ids=True):
        """Fused gather+FM kernel emitting x, then the tower kernel."""
        dense, ids = _split_criteo(inputs, self.nd, self._dev)
        B = ids.shape[0]
        x = torch.empty(B, self.nd + self.embed_layer.n_fields * self.embed_layer.k, dtype=torch.float32,
                        device=self._dev)
        fm = self.fm_logit((dense, ids), x_out=x, check_ids=check_ids)
        if self.dnn.output_layer.units == 1 and self.dnn.tower_ok():
            # DNN tower + sigmoid(0.5*fm + 0.5*dnn) head in one launch
            return self.dnn.tower(x, extra=fm, c0=0.5, c1=0.5, head=True)
        dnn = self.dnn(x)
        return sigmoid_combine(fm, dnn, 0.5, 0.5)


class DCN(KerasModule):
    """DCN — model/dcn.py:15-34: sigmoid(Dense1([CrossLayer(x) | DNNLayer(x)]))."""

    def __init__(self, feature_columns, hidden_units, output_dim, activation, layer_num, reg_w=1e-4, reg_b=1e-4,
                 embed_dim=8, device=None, seed=None):
        super().__init__(device, seed)
        self.dense_feature_columns, self.sparse_feature_columns = feature_columns
        self.nd = len(self.dense_feature_columns)
        self.embed_layer = EmbedLayer(self.sparse_feature_columns, embed_dim, device=device, seed=_subseed(self._gen))
        d = self.nd + self.embed_layer.n_fields * embed_dim
        self.dense_layer = DNNLayer(hidden_units, output_dim, activation, device=device, seed=_subseed(self._gen))
        self.dense_layer.build(d)
        self.cross_layer = CrossLayer(layer_num, reg_w, reg_b, device=device, seed=_subseed(self._gen), input_dim=d)
        # Dense(1) followed by tf.nn.sigmoid (model/dcn.py:33): the sigmoid is
        # fused into the Dense epilogue; weights keep the Keras Dense names.
        self.output_layer = Dense(1, "sigmoid", device=device, seed=_subseed(self._gen), input_dim=d + output_dim)
        self.d = d
        self._err = _ErrFlag(self._dev)

    def cross_fused(self, inputs, out=None, check_ids=True):
        """CrossLayer([dense | EmbedLayer(ids)]) in ONE launch (rs_embed_cross_fwd):
        x0 is assembled in LDS and never written to HBM."""
        dense, ids = _split_criteo(inputs, self.nd, self._dev)
        B = ids.shape[0]
        e = self.embed_layer
        if out is None:
            out = torch.empty(B, self.d, dtype=torch.float32, device=self._dev)
        prep = self.cross_layer.prepared(self.d)
        hoff, hvoc = e.host_meta()  # field metadata also by value (the kernel-argument front end)
        call("rs_embed_cross_fwd_hm", ptr(ids), _lib.id_kind(ids), ids.stride(0), ptr(dense), dense.stride(0),
             self.nd, ptr(e.table), ptr(e.field_offsets), ptr(e.field_vocab), hoff, hvoc, e.n_fields, e.k,
             self.cross_layer.layer_num, ptr(prep), ptr(out), out.stride(0), B, ptr(self._err.t), _lib.stream())
        if check_ids:
            self._err.check("DCN")
        return out

    def train_step(self, inputs, labels, lr=0.01, return_loss=False, check_ids=True, dropout=None):
        """One step of compile_fit on DCN (model/dcn.py:24-34, utils/compile_fit.py:
        9-15): SGD(lr), binary cross-entropy on sigmoid(Dense1([CrossLayer(x) |
        DNNLayer(x)])), CrossLayer's l2(reg_w) / l2(reg_b) regularisers
        (layer/interaction.py:57-73), every weight updated in place from the
        pre-step gradients.  The CrossNet runs as rs_cross_train_fwd (keeps
        x_1..x_L and x_l . w_l) and rs_cross_train_bwd (delta_l recursion);
        dw_l = x_l^T s_l and the Dense grads through rs_gemm, db_l / Dense
        biases through rs_col_sum, the looked-up rows by rs_embedding_sgd.
        DNNLayer's Dropout runs in training mode (counter-based masks,
        rs_dropout; dropout=False turns it off), as DeepFM.train_step."""
        dense, ids = _split_criteo(inputs, self.nd, self._dev)
        labels = _to_device_f32(labels, self._dev).reshape(-1)
        e, cl, dnn, out = self.embed_layer, self.cross_layer, self.dense_layer, self.output_layer
        rate = _dropout_rate(dnn, dropout)
        _check_train_tower("DCN", dnn)
        B, d, dev, st = ids.shape[0], self.d, self._dev, _lib.stream()
        od, Lc = dnn.output_layer.units, cl.layer_num
        dz_n = d + od
        emp = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
        layers = list(dnn.hidden_layer) + [dnn.output_layer]
        gw = gemm_ws(self, gemm_need([(*L.kernel.shape, B) for L in layers] + [(d, 1, B), (dz_n, 1, B)]))
        # forward, keeping what the backward needs
        x = e.gather(ids, dense, check_ids=check_ids)
        zc = emp(B, dz_n)  # [cross_out | dnn_out], the output Dense's input
        W = torch.stack([w.reshape(-1) for w in cl.cross_weight]).contiguous() if Lc else None
        Bc = torch.stack([b.reshape(-1) for b in cl.cross_bias]).contiguous() if Lc else None
        xs, gl = (emp(Lc, B, d), emp(Lc, B)) if Lc else (None, None)
        if Lc:
            call("rs_cross_train_fwd", ptr(x), d, d, Lc, ptr(W), ptr(Bc), B, ptr(xs), ptr(gl), ptr(zc), dz_n, st)
        else:
            zc[:, :d].copy_(x)
        acts, drop = _dnn_train_forward(self, dnn, x, rate, st)
        dnn.output_layer(acts[-1], out=zc[:, d:])
        logit = emp(B)
        call("rs_dense_fwd", ptr(zc), dz_n, ptr(out.kernel), ptr(out.bias), None, 0, ptr(logit), 1, B, dz_n, 1, st)
        g, loss = bce_head_logit(logit, labels, return_loss, st)
        # output Dense: dWo = zc^T g, dbo = sum g, dzc = g Wo^T
        dWo, dbo, dzc = dense_backward(out.kernel, zc, g.view(B, 1), gw, emp, st)
        # DNN backward from dzc[:, d:], then the CrossNet's from dzc[:, :d]
        grads, dx = _dnn_backward(layers, acts, dzc[:, d:], gw, emp, st, drop=drop)
        if Lc:
            deltas, sl = emp(Lc, B, d), emp(Lc, B)
        else:
            deltas = sl = None
        call("rs_cross_train_bwd", ptr(x), d, d, Lc, ptr(W), B, ptr(gl), ptr(dzc), dz_n, ptr(deltas), ptr(sl),
             ptr(dx), d, st)
        dWc, dBc = emp(max(Lc, 1), d), emp(max(Lc, 1), d)
        for l in range(Lc):
            xl = x if l == 0 else xs[l - 1]
            call("rs_gemm", 1, 0, d, 1, B, 1.0, ptr(xl), d, ptr(sl[l]), 1, 0.0, ptr(dWc[l]), 1, None, 0, *gw, st)
            call("rs_col_sum", ptr(deltas[l]), d, B, d, ptr(dBc[l]), st)
        # updates
        upd = _dnn_updates(grads) + [(out.kernel, dWo, dz_n, 0.0), (out.bias, dbo, 1, 0.0)]
        for l in range(Lc):
            upd += [(cl.cross_weight[l], dWc[l], d, cl.reg_w), (cl.cross_bias[l], dBc[l], d, cl.reg_b)]
        _lib.sgd_update_multi(upd, lr, st)
        embedding_sgd(e, ids, ptr(dx) + 4 * self.nd, d, lr, st, self)
        self.__dict__["_keep"] = (W, Bc)  # stream-ordered lifetime of the stacked operands
        self._weights_changed()
        return loss

    # ---- one-launch forward (rs_dcn_fwd)
    def _fused_layers(self):
        dl = self.dense_layer
        return list(dl.hidden_layer), dl.output_layer

    def fused_ok(self):
        hidden, last = self._fused_layers()
        if any(l.activation not in (None, "linear", "relu", "prelu", "sigmoid") for l in hidden):
            return False
        dims = [self.d] + [l.units for l in hidden] + [1]
        e = self.embed_layer
        return bool(_lib.lib().rs_dcn_fused_ok(self.nd, e.n_fields, e.k, self.cross_layer.layer_num, len(dims) - 1,
                                                ints(dims)))

    def _fused_params(self):
        """Cross image over [w_0..w_{L-1}, w_o[:d]] and the DNN tower with its
        last layer folded with the output Dense's DNN half (cached)."""
        hidden, last = self._fused_layers()
        out = self.output_layer
        cl = self.cross_layer
        params = list(cl.cross_weight) + list(cl.cross_bias) + [out.kernel, out.bias, last.kernel, last.bias] + \
            [p for l in hidden for p in (l.kernel, l.bias, l.alpha) if p is not None]
        d = self.d

        @torch.no_grad()
        def build():
            L = cl.layer_num
            W = torch.cat([w.reshape(1, d) for w in cl.cross_weight] + [out.kernel[:d].reshape(1, d)]).contiguous()
            Bb = torch.cat([b.reshape(1, d) for b in cl.cross_bias] + [torch.zeros(1, d, device=self._dev)]).contiguous()
            cross = sized("rs_cross_prepared_size", d, L + 1, device=self._dev)
            call("rs_cross_prepare", ptr(W), ptr(Bb), d, L + 1, ptr(cross), _lib.stream())
            # fold on rs_dense_fwd: wf = last.kernel @ wo2, bf = last.bias @ wo2 + out.bias
            wo2 = out.kernel[d:].reshape(-1, 1).contiguous()          # [out_dim, 1]
            h_last, od = last.kernel.shape
            kern = last.kernel.contiguous()
            wf = torch.empty(h_last, 1, dtype=torch.float32, device=self._dev)
            bf = torch.empty(1, dtype=torch.float32, device=self._dev)
            st = _lib.stream()
            call("rs_dense_fwd", ptr(kern), od, ptr(wo2), None, None, _lib.ACT[None], ptr(wf), 1, h_last, od, 1, st)
            call("rs_dense_fwd", ptr(last.bias), od, ptr(wo2), ptr(out.bias), None, _lib.ACT[None], ptr(bf), 1, 1, od, 1,
                 st)
            ks = [l.kernel for l in hidden] + [wf]
            bs = [l.bias for l in hidden] + [bf.contiguous()]
            als = [l.alpha for l in hidden] + [None]
            dims = [d] + [l.units for l in hidden] + [1]
            nl, ci = len(ks), ints(dims)
            mlp = sized("rs_mlp_prepared_size", nl, ci, device=self._dev)
            call("rs_mlp_prepare", nl, ci, ptrs(ks), ptrs(bs), ptrs(als), None, ptr(mlp), _lib.stream())
            acts = [_lib.ACT[l.activation] for l in hidden] + [0]
            return cross, mlp, dims, acts, (W, Bb, wf, bf)
        return self._packed("dcn", params, build)

    def forward_fused(self, inputs, check_ids=True):
        """DCN.call as ONE kernel (rs_dcn_fwd)."""
        dense, ids = _split_criteo(inputs, self.nd, self._dev)
        B = ids.shape[0]
        e = self.embed_layer
        cross, mlp, dims, acts, _ = self._fused_params()
        n = len(dims) - 1
        out = torch.empty(B, 1, dtype=torch.float32, device=self._dev)
        hoff, hvoc = e.host_meta()
        call("rs_dcn_fwd_hm", ptr(ids), _lib.id_kind(ids), ids.stride(0), ptr(dense), dense.stride(0), self.nd,
             ptr(e.table), ptr(e.field_offsets), ptr(e.field_vocab), hoff, hvoc, e.n_fields, e.k,
             self.cross_layer.layer_num, ptr(cross), n, ints(dims), ints(acts), ptr(mlp),
             ptr(out), B, ptr(self._err.t), _lib.stream())
        if check_ids:
            self._err.check("DCN")
        return out

    def forward(self, inputs, check_ids=True):
        if self.fused_ok():
            return self.forward_fused(inputs, check_ids)
        return self.forward_unfused(inputs, check_ids)

    def forward_unfused(self, inputs, check_ids=True):
        dense, ids = _split_criteo(inputs, self.nd, self._dev)
        x = self.embed_layer.gather(ids, dense=dense, check_ids=check_ids)
        B = x.shape[0]
        z = torch.empty(B, self.d + self.dense_layer.output_layer.units, dtype=torch.float32, device=self._dev)
        self.cross_layer(x, out=z[:, :self.d])
        if self.dense_layer.tower_ok():
            self.dense_layer.tower(x, out=z[:, self.d:])
        else:
            h = x
            for layer in self.dense_layer.hidden_layer:
                h = layer(h)
            self.dense_layer.output_layer(h, out=z[:, self.d:])
        return self.output_layer(z)


class PNN(KerasModule):
    """PNN(feature_columns, mode, ...) — model/pnn.py:14-53, with 3-D
    embeddings (the reference reshapes them to 2-D before the product layers
    and crashes at :38).  mode 'inner' / 'outer' / 'both'; the DNN input
    [flat_emb | inner | outer] comes out of ONE launch (rs_embed_product_fwd).
    use_fgcnn=True: the products and the flat part run on z = concat([embed,
    FGCNNLayer(embed)], axis=1) (model/pnn.py:33-36) — the conv stack from the
    ids (which also gathers embed into z), one Dense per FGCNN layer into z,
    then rs_product_fwd on z; ``fgcnn`` (a dict) passes FGCNNLayer's
    arguments.  Returns the DNN logit (no sigmoid, as the reference).

    ``train_fgcnn`` (default False; True needs use_fgcnn=True, else
    ValueError): with the default a use_fgcnn model refuses ``train_step`` /
    ``gradients`` (NotImplementedError).  Training it is an opt-in because it
    is a deviation: the reference builds FGCNN's recombination Dense layers
    inside ``call`` (layer/interaction.py:253), so in its loop (model/pnn.py:
    74-81) they are redrawn on every call and are not in model.variables —
    the literal step never trains them and is not reproducible.  The forward
    here already builds them once; train_fgcnn=True extends that to training:
    conv kernels and biases, recombination kernels and biases, the DNN, the
    outer-product W and the looked-up table rows all take the SGD step.
    Limits: n_z <= 128 fields, k in {4, 8, 16}, and the conv backward's LDS
    tile (rs_fgcnn_conv_bwd_workspace_size); anything else raises
    NotImplementedError before any launch."""

    def __init__(self, feature_columns, mode, hidden_units, output_dim, activation="relu", dropout=0.2,
                 use_fgcnn=False, embed_dim=8, device=None, seed=None, fgcnn=None, train_fgcnn=False):
        super().__init__(device, seed)
        if mode not in ("inner", "outer", "both"):
            raise ValueError("Please choice mode's value in 'inner', 'outer', 'both'.")
        self.use_fgcnn = bool(use_fgcnn)
        self.train_fgcnn = bool(train_fgcnn)
        if self.train_fgcnn and not self.use_fgcnn:
            raise ValueError("PNN train_fgcnn=True needs use_fgcnn=True")
        if self.use_fgcnn and self._dev.type != "cuda":
            # FGCNN exists only as HIP kernels; a model built for another device
            # could never run it, so it is refused when it is built
            raise NotImplementedError("PNN use_fgcnn=True: FGCNNLayer runs only on a HIP device "
                                      f"(device={self._dev})")
        self.mode = mode
        self.dense_feature_columns, self.sparse_feature_columns = feature_columns
        self.nd = len(self.dense_feature_columns)
        self.embed_layer = EmbedLayer(self.sparse_feature_columns, embed_dim, device=device, seed=_subseed(self._gen))
        F = self.embed_layer.n_fields
        self.inner_product_layer = InnerProductLayer(device=device)
        self.outer_product_layer = OuterProductLayer(device=device, seed=_subseed(self._gen))
        dnn_seed = _subseed(self._gen)
        if self.use_fgcnn:
            self.fgcnn_layer = FGCNNLayer(**(fgcnn or {}), device=device, seed=_subseed(self._gen))
            self.fgcnn_layer.build(F, embed_dim)
            F += self.fgcnn_layer.n_new  # the product layers and the flat part see z
        self.n_z = F
        P = F * (F - 1) // 2
        if mode != "inner":
            self.outer_product_layer.build(F, embed_dim)
        self.width = F * embed_dim + P * (2 if mode == "both" else 1)
        self.dnn_layer = DNNLayer(hidden_units, output_dim, activation, dropout, device=device, seed=dnn_seed)
        self.dnn_layer.build(self.width)
        self._err = _ErrFlag(self._dev)

    def product_inputs(self, inputs, check_ids=True, keep=None):
        """[flat_emb | inner | outer] (model/pnn.py:37-48) in one launch.
        ``keep`` (a dict, use_fgcnn only) receives what the backward reads: z
        and the conv stack's workspace ws."""
        _, ids = _split_criteo(inputs, self.nd, self._dev)
        e = self.embed_layer
        B = ids.shape[0]
        out = torch.empty(B, self.width, dtype=torch.float32, device=self._dev)
        if self.use_fgcnn:
            # z = [embed | fgcnn_out] [B, F', k]: the conv launch gathers embed into
            # z and fills the pooled maps, each layer's Dense writes its new fields
            # into z, then [flat | inner | outer] of z in one launch
            fg = self.fgcnn_layer
            z = torch.empty(B, self.n_z * e.k, dtype=torch.float32, device=self._dev)
            ws = fg.conv_ids(ids, e, z, self._err.t)
            fg.recombine(ws, z, col=e.n_fields * e.k)
            call("rs_product_fwd", ptr(z), self.n_z, e.k, 1 if self.mode != "outer" else 0,
                 ptr(self.outer_product_layer.prepared()) if self.mode != "inner" else None, ptr(out),
                 out.stride(0), B, _lib.stream())
            if check_ids:
                self._err.check("PNN")
            if keep is not None:
                keep["z"], keep["ws"] = z, ws
            return out
        hoff, hvoc = e.host_meta()  # field metadata also by value (the kernel-argument front end)
        if self.mode == "inner":
            call("rs_embed_inner_fwd_hm", ptr(ids), _lib.id_kind(ids), ids.stride(0), ptr(e.table),
                 ptr(e.field_offsets), ptr(e.field_vocab), hoff, hvoc, e.n_fields, e.k, ptr(out), out.stride(0), B,
                 ptr(self._err.t), _lib.stream())
        else:
            call("rs_embed_product_fwd_hm", ptr(ids), _lib.id_kind(ids), ids.stride(0), ptr(e.table),
                 ptr(e.field_offsets), ptr(e.field_vocab), hoff, hvoc, e.n_fields, e.k,
                 1 if self.mode == "both" else 0, ptr(self.outer_product_layer.prepared()), ptr(out), out.stride(0),
                 B, ptr(self._err.t), _lib.stream())
        if check_ids:
            self._err.check("PNN")
        return out

    def forward(self, inputs, check_ids=True):
        return self.dnn_layer(self.product_inputs(inputs, check_ids))

    def train_step(self, inputs, labels, lr=0.01, return_loss=False, check_ids=True):
        """One step of the reference's own PNN loop (model/pnn.py:74-81:
        GradientTape, SGD(lr) over model.variables, loss
        tf.reduce_mean(losses.binary_crossentropy(y_train, pre)) on the DNN
        LOGIT — Keras' clipped probability form with the labels broadcast
        against the [B, 1] output, rs_bce_prob_grad), modes 'inner' /
        'outer' / 'both' (the loop's own example runs 'both', :61):
          [flat | inner | outer] in one launch (rs_embed_inner_fwd /
          rs_embed_product_fwd), DNN forward with saved activations
          (rs_dense_fwd), the DNN backward (split-K rs_gemm, rs_col_sum),
          rs_inner_product_bwd (dflat + sum_j dinner_ij e_j),
          rs_outer_product_bwd (+ sum g_p e_j W_p / e_i W_p^T) and
          rs_outer_product_w_grad (dW), then SGD of the DNN and of W and
          row-sparse rs_embedding_sgd of the tables.  The loop's loss has no
          regulariser (OuterProductLayer's l2 sits in model.losses, never
          added there).  The loop calls model(X) without training=True, so
          Dropout is the identity there too.  Returns the per-sample losses
          (before the step) if ``return_loss``.

        use_fgcnn=True trains only a model built with ``train_fgcnn=True``
        (see the class docstring); then ``gradients`` also runs
        rs_product_bwd / rs_product_w_grad on z and FGCNNLayer.backward, and
        the conv kernels and biases and the recombination kernels and biases
        take the same SGD step.  A bad id raises before any weight moves."""
        grads, loss, ids = self._gradients(inputs, labels, check_ids, return_loss, "train_step")
        names = dict(self.named_parameters())
        de = grads.pop("embed_rows")
        if ids.shape[0] == 0 and self.use_fgcnn:
            return loss
        st = _lib.stream()
        _lib.sgd_update_multi([(names[n], g, g.numel(), 0.0) for n, g in grads.items()], lr, st)
        embedding_sgd(self.embed_layer, ids, ptr(de), de.stride(0), lr, st, self)
        self._weights_changed()
        return loss

    def gradients(self, inputs, labels, check_ids=True):
        """The gradients of one ``train_step``'s loss, with no weight changed:
        ({name: gradient} keyed like ``named_parameters()`` for every dense
        tensor, plus "embed_rows": dL/d(looked-up rows) [B, F, k] per sample,
        before the scatter into the table; the per-sample losses [B])."""
        grads, loss, _ = self._gradients(inputs, labels, check_ids, True, "gradients")
        e = self.embed_layer
        grads["embed_rows"] = grads["embed_rows"].view(-1, e.n_fields, e.k)
        return grads, loss

    def _check_train(self, what):
        dnn = self.dnn_layer
        if self.use_fgcnn and not self.train_fgcnn:
            raise NotImplementedError(f"PNN.{what}: use_fgcnn trains only a model built with train_fgcnn=True")
        if dnn.output_layer.units != 1:
            raise NotImplementedError(f"PNN.{what}: output_dim 1 only")
        _check_train_tower("PNN", dnn)
        if self.use_fgcnn:
            if self.n_z > 128 or self.embed_layer.k not in (4, 8, 16):
                raise NotImplementedError(f"PNN.{what}: use_fgcnn trains up to 128 fields of z (got {self.n_z}) "
                                          f"and k in {{4, 8, 16}} (got {self.embed_layer.k})")
            try:
                self.fgcnn_layer.bwd_workspace_size(1)
            except _lib.RSError as err:
                raise NotImplementedError(f"PNN.{what}: {err}") from None

    def _gradients(self, inputs, labels, check_ids, want_loss, what):
        """({parameter name: gradient, "embed_rows": [B, F*k]}, losses or None,
        ids) — the launches of one step up to, not including, the updates."""
        self._check_train(what)
        dnn = self.dnn_layer
        _, ids = _split_criteo(inputs, self.nd, self._dev)
        labels = _to_device_f32(labels, self._dev).reshape(-1)
        e = self.embed_layer
        B, F, k, st = ids.shape[0], e.n_fields, e.k, _lib.stream()
        emp = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=self._dev)
        name_of = {id(p): n for n, p in self.named_parameters()}
        if self.use_fgcnn and B == 0:  # nothing to launch: zero gradients, no losses
            grads = {n: torch.zeros_like(p) for n, p in self.named_parameters() if p is not e.table}
            grads["embed_rows"] = emp(0, F * k)
            return grads, emp(0) if want_loss else None, ids
        keep = {} if self.use_fgcnn else None
        x = self.product_inputs(inputs, check_ids, keep=keep)  # [B, width]: [flat | inner | outer]
        layers = list(dnn.hidden_layer) + [dnn.output_layer]
        acts, _ = _dnn_train_forward(self, dnn, x, 0.0, st)  # (rate 0: no draw, as the loop)
        pre = dnn.output_layer(acts[-1])
        g = emp(B)
        loss = emp(B) if want_loss else None
        call("rs_bce_prob_grad", ptr(pre), pre.stride(0), ptr(labels), B, ptr(g), ptr(loss), st)
        gw = gemm_ws(self, gemm_need([(*L.kernel.shape, B) for L in layers]))
        dgrads, delta = _dnn_backward(layers, acts, g.view(B, 1), gw, emp, st)
        grads = {}
        for L, dW, db in dgrads:
            grads[name_of[id(L.kernel)]], grads[name_of[id(L.bias)]] = dW, db
        w = self.width
        op = self.outer_product_layer
        outer, inner = self.mode != "inner", self.mode != "outer"
        de = emp(B, F * k)
        if self.use_fgcnn:
            # dz [B, n_z*k] of [flat | inner | outer] in one launch; its new-field
            # columns go back through FGCNNLayer, whose dL/d(rows) joins the first F*k
            z, nz = keep["z"], self.n_z
            dz = emp(B, nz * k)
            call("rs_product_bwd", ptr(z), z.stride(0), ptr(delta), w, nz, k, 1 if inner else 0,
                 ptr(op.W) if outer else None, B, ptr(dz), dz.stride(0), st)
            if outer:
                dW = emp(*op.W.shape)
                call("rs_product_w_grad", ptr(z), z.stride(0), ptr(delta), w, nz, k, 1 if inner else 0, B, ptr(dW), st)
                grads[name_of[id(op.W)]] = dW
            de.copy_(dz[:, :F * k])
            fg = self.fgcnn_layer
            fgrads = fg.backward(z, keep["ws"], z[:, F * k:], dz[:, F * k:], de)
            for n, p in fg.keras_weights().items():
                grads[name_of[id(p)]] = fgrads[n]
            grads["embed_rows"] = de
            return grads, loss, ids
        P = F * (F - 1) // 2
        if inner:
            call("rs_inner_product_bwd", ptr(x), w, ptr(delta) + 4 * F * k, w, ptr(delta), w, F, k, B, ptr(de),
                 F * k, st)
        else:
            de.copy_(delta[:, :F * k])
        if outer:
            o0 = F * k + (P if self.mode == "both" else 0)  # the outer block's first column
            dW = emp(*op.W.shape)
            call("rs_outer_product_bwd", ptr(x), w, ptr(delta) + 4 * o0, w, ptr(op.W), F, k, B, ptr(de), F * k, st)
            call("rs_outer_product_w_grad", ptr(x), w, ptr(delta) + 4 * o0, w, F, k, B, ptr(dW), st)
            grads[name_of[id(op.W)]] = dW
        grads["embed_rows"] = de
        return grads, loss, ids


class DIN(TowerMixin, KerasModule):
    """DIN — model/din.py:15-95.  ``forward(inputs)`` takes the reference's
    dict: each dense / non-behaviour sparse feature [B,1] (or [B]), each
    behaviour feature [B,T] (0 = padding), and the candidate under the
    hard-coded key 'movie_id' (model/din.py:74) as [B, n_behaviour]: column i
    is the candidate's id for behaviour feature i (e.g. item id and category
    id, :73,77-79).  Behaviour features are taken in sparse-column order; their
    embeddings are concatenated along k and the mask comes from the first
    (:80)."""

    # train_step: the two-layer PReLU attention unit's forward and backward as
    # one launch each (rs_din_att_prelu_fwd / _bwd; False: the layer-by-layer
    # kernels; both are tested vs the oracle)
    fused_att_train = True

    def __init__(self, feature_columns, behavior_feature_list, att_hidden_units=(80, 40),
                 dnn_hidden_units=(256, 128, 64), att_attention="prelu", dnn_activation="prelu", dnn_dropout=0.0,
                 device=None, seed=None):
        super().__init__(device, seed)
        self.dense_feature_columns, self.sparse_feature_columns = feature_columns
        self.behavior_feature_list = list(behavior_feature_list)
        self.other_sparse = [f for f in self.sparse_feature_columns if f["feat"] not in self.behavior_feature_list]
        self.seq_feats = [f for f in self.sparse_feature_columns if f["feat"] in self.behavior_feature_list]
        if not self.seq_feats:
            raise ValueError("DIN: behavior_feature_list names no sparse feature column")
        self.other_sparse_num = len(self.other_sparse)
        self.dense_num = len(self.dense_feature_columns)
        self.behavior_num = len(self.behavior_feature_list)
        dev = device
        self.embed_sparse_layers = torch.nn.ModuleList(
            [EmbedLayer([f], k=f["embed_dim"], device=dev, seed=_subseed(self._gen)) for f in self.other_sparse])
        self.embed_seq_layers = torch.nn.ModuleList(
            [EmbedLayer([f], k=f["embed_dim"], device=dev, seed=_subseed(self._gen)) for f in self.seq_feats])
        self.att_layer = Attention(att_hidden_units, att_attention, device=dev, seed=_subseed(self._gen))
        self.bn_layer = BatchNormalization(device=dev)
        act = "prelu" if dnn_activation == "prelu" else "dice"
        self.dense_layer = torch.nn.ModuleList(
            [Dense(u, activation=act, device=dev, seed=_subseed(self._gen)) for u in dnn_hidden_units])
        self.dropout = dnn_dropout
        self.out_layer = Dense(1, activation="sigmoid", device=dev, seed=_subseed(self._gen))
        self._err = _ErrFlag(self._dev)

    def _behaviour_embed(self, ids_cols, rows, check_ids):
        """[rows, K] = concat_i embed_seq_layers[i](ids_cols[i]) along k."""
        K = sum(l.k for l in self.embed_seq_layers)
        out = torch.empty(rows, K, dtype=torch.float32, device=self._dev)
        col = 0
        for ids, layer in zip(ids_cols, self.embed_seq_layers):
            layer.gather(ids, out=out[:, col:col + layer.k], check_ids=check_ids)
            col += layer.k
        return out

    def forward(self, inputs, check_ids=True):
        dev = self._dev
        nb = len(self.seq_feats)
        hists = [_ids_tensor(inputs[f["feat"]], dev) for f in self.seq_feats]
        B, T = hists[0].shape
        if any(h.shape != (B, T) for h in hists):
            raise ValueError("DIN: every behaviour feature must be [B, T]")
        cand = _ids_tensor(inputs["movie_id"], dev).reshape(B, -1)
        if cand.shape[1] != nb:
            raise ValueError(f"DIN: inputs['movie_id'] needs one candidate id per behaviour feature ({nb})")
        K = sum(l.k for l in self.embed_seq_layers)
        other_k = sum(l.k for l in self.embed_sparse_layers)
        width = 2 * K + other_k + self.dense_num
        emb = torch.empty(B, width, dtype=torch.float32, device=dev)
        if self.att_layer.out_kernel is None:
            self.att_layer.build(T, K)
        if nb == 1 and self.att_layer.ids_ok(K) and self.fused_call:
            y = self._forward_one_launch(inputs, hists[0], cand, K, width, check_ids)
            if y is not None:
                return y
        if nb == 1 and self.att_layer.ids_ok(K):
            # keys/values read through the ids from the (L2-resident) table; the
            # pooled rows and the candidate rows go straight into emb, in the
            # attention's one launch (rs_din_attention_ids_cand_fwd)
            seq_layer = self.embed_seq_layers[0]
            self.att_layer.forward_ids(seq_layer.table, int(seq_layer.vocab_sizes[0]), hists[0], cand,
                                       err=self._err.t, out=emb[:, :K], cand_out=emb[:, K:2 * K])
            if check_ids:
                self._err.check("DIN")
        else:
            item_embed = self._behaviour_embed([cand[:, i:i + 1] for i in range(nb)], B, check_ids)
            seq_embed = self._behaviour_embed([h.reshape(B * T, 1) for h in hists], B * T, check_ids)
            seq_embed = seq_embed.view(B, T, K)
            mask = (hists[0] != 0).to(torch.float32)  # model/din.py:80: the first behaviour feature
            att_emb = self.att_layer([item_embed, seq_embed, seq_embed, mask])
            emb[:, K:2 * K] = item_embed
            emb[:, :K] = att_emb
        if self.out_layer.kernel is not None and self.tower_ok():
            # BatchNormalization + PReLU MLP + Dense(1, sigmoid) in one launch,
            # the other sparse embeddings and the dense features read
            # straight into its input tile (no concat launch, no buffer)
            if self.bn_layer.gamma is None:
                self.bn_layer.build(emb.shape[-1])
            pieces = self._rest_pieces(inputs, 2 * K, B)
            if self.pieces_in_tower and 0 < len(pieces) <= 16 and width <= 64:
                y = self._tower_pieces(emb, pieces, self.bn_layer.affine())
                if check_ids:
                    self._err.check("DIN")
                return y
            self._concat_rest(inputs, emb, 2 * K, B, check_ids)
            return self.tower(emb, in_affine=self.bn_layer.affine())
        self._concat_rest(inputs, emb, 2 * K, B, check_ids)
        x = self.bn_layer(emb)
        for layer in self.dense_layer:
            x = layer(x)
        return self.out_layer(x)

    # DIN.call from the ids to the logit as ONE launch (rs_din_forward_ids:
    # the attention unit, then bn + the PReLU tower + Dense(1, sigmoid) in the
    # same workgroups; bit-identical to the two launches below, which stay the
    # path for shapes it does not take and for fused_call = False)
    fused_call = True

    def _forward_one_launch(self, inputs, hist, cand, K, width, check_ids):
        if self.out_layer.kernel is None or not self.tower_ok() or not self.pieces_in_tower or width > 64:
            return None
        B, T = hist.shape
        pieces = self._rest_pieces(inputs, 2 * K, B)
        if not 0 < len(pieces) <= 16:
            return None
        att = self.att_layer
        if att.out_kernel is None:
            att.build(T, K)
        h1, h2 = att.hidden_units
        ls = self._layers()
        n = len(ls)
        dims = self._dims()
        cdims = ints(dims)
        if T != att.T or not _lib.lib().rs_din_forward_ids_supported(T, K, h1, h2, n, cdims):
            return None
        if self.bn_layer.gamma is None:
            self.bn_layer.build(width)
        sc, sh = self.bn_layer.affine()
        seq_layer = self.embed_seq_layers[0]
        y = torch.empty(B, 1, dtype=torch.float32, device=self._dev)
        k = len(pieces)
        arr = lambda ctype, vals: (ctype * k)(*vals)
        call("rs_din_forward_ids", ptr(hist), _lib.id_kind(hist), hist.stride(0), ptr(cand), cand.stride(0), T, K,
             ptr(seq_layer.table), int(seq_layer.vocab_sizes[0]), h1, h2, ptr(att.prepared_ids(K)), None, 0,
             ptr(sc), ptr(sh), n, cdims, ints([_lib.ACT[l.activation] for l in ls]),
             ptr(self.prepared()), ptr(y), y.stride(0), k, arr(C.c_int, [p[0] for p in pieces]),
             arr(C.c_int, [p[1] for p in pieces]), arr(C.c_int, [p[2] for p in pieces]),
             arr(C.c_void_p, [ptr(p[3]) for p in pieces]), arr(C.c_int64, [p[3].stride(0) for p in pieces]),
             arr(C.c_void_p, [ptr(p[4]) if p[4] is not None else None for p in pieces]),
             arr(C.c_int64, [p[5] for p in pieces]), B, ptr(self._err.t), _lib.stream())
        if check_ids:
            self._err.check("DIN")
        return y

    # DIN.call's tower reads the other sparse embeddings and the dense
    # features itself (rs_mlp_affine_pieces_fwd); False: one rs_concat_pieces
    # launch writes them into the concat first (both tested)
    pieces_in_tower = True

    def _rest_pieces(self, inputs, col, B):
        """(width, column, kind, source, table, vocab) of the other sparse
        embeddings and the dense features, from column `col` on
        (model/din.py:64-69,84-85)."""
        dev = self._dev
        pieces = []
        for f, layer in zip(self.other_sparse, self.embed_sparse_layers):
            ids = _ids_tensor(inputs[f["feat"]], dev).reshape(B, 1)
            pieces.append((layer.k, col, _lib.id_kind(ids), ids, layer.table, int(layer.vocab_sizes[0])))
            col += layer.k
        for f in self.dense_feature_columns:
            x = _to_device_f32(inputs[f["feat"]], dev).reshape(B, 1)
            pieces.append((1, col, -1, x, None, 0))
            col += 1
        return pieces

    def _tower_pieces(self, emb, pieces, affine):
        """BN + PReLU MLP + head over [emb[:, :2K] | pieces] in one launch."""
        ls = self._layers()
        n = len(ls)
        dims = self._dims()
        B = emb.shape[0]
        out = torch.empty(B, dims[-1], dtype=torch.float32, device=self._dev)
        sc, sh = affine
        k = len(pieces)
        arr = lambda ctype, vals: (ctype * k)(*vals)
        call("rs_mlp_affine_pieces_fwd", ptr(emb), emb.stride(0), ptr(sc), ptr(sh), n, ints(dims),
             ints([_lib.ACT[l.activation] for l in ls]), ptr(self.prepared()), ptr(out), out.stride(0), 0,
             None, 1.0, 1.0, B, k, arr(C.c_int, [p[0] for p in pieces]), arr(C.c_int, [p[1] for p in pieces]),
             arr(C.c_int, [p[2] for p in pieces]), arr(C.c_void_p, [ptr(p[3]) for p in pieces]),
             arr(C.c_int64, [p[3].stride(0) for p in pieces]),
             arr(C.c_void_p, [ptr(p[4]) if p[4] is not None else None for p in pieces]),
             arr(C.c_int64, [p[5] for p in pieces]), ptr(self._err.t), _lib.stream())
        return out

    def _concat_rest(self, inputs, emb, col, B, check_ids):
        """The other sparse embeddings and the dense features into emb[:, col:]
        (model/din.py:64-69,84-85): ONE rs_concat_pieces launch for up to 16
        pieces, one launch per piece beyond."""
        pieces = self._rest_pieces(inputs, col, B)
        for i in range(0, len(pieces), 16):
            part = pieces[i:i + 16]
            n = len(part)
            arr = lambda ctype, vals: (ctype * n)(*vals)
            call("rs_concat_pieces", n, arr(C.c_int, [p[0] for p in part]), arr(C.c_int, [p[1] for p in part]),
                 arr(C.c_int, [p[2] for p in part]), arr(C.c_void_p, [ptr(p[3]) for p in part]),
                 arr(C.c_int64, [p[3].stride(0) for p in part]),
                 arr(C.c_void_p, [ptr(p[4]) if p[4] is not None else None for p in part]),
                 arr(C.c_int64, [p[5] for p in part]), ptr(emb), emb.stride(0), B, ptr(self._err.t), _lib.stream())
        if check_ids and pieces:
            self._err.check("DIN")

    def _layers(self):
        return list(self.dense_layer) + [self.out_layer]

    def train_step(self, inputs, labels, lr=0.01, return_loss=False, check_ids=True, dropout=None):
        """One step of compile_fit on DIN (utils/compile_fit.py:9-15: Keras
        fit, SGD(lr), binary_crossentropy on the sigmoid output — Keras takes
        the sigmoid's logit) with DIN.call in training mode (model/din.py:
        56-95): BatchNormalization normalises with the batch's own mean and
        biased variance and moves its averages (momentum 0.99), and so do
        the Dice layers' BatchNormalizations (att_attention / dnn_activation
        'prelu' — the reference defaults — or 'dice': rs_dice_train_fwd/_bwd).
          forward: behaviour / candidate rows (rs_embed_gather), the
          attention input [q, k, q-k, q*k] (rs_din_att_concat), each
          attention Dense (rs_dense_fwd) + PReLU over [T, h] alphas
          (rs_prelu_rows_fwd, kept pre-activations), the score Dense, masked
          softmax + pool (rs_masked_softmax_pool), rs_bn_train_fwd, the PReLU
          DNN and the output logit;
          backward: rs_head_grad, per Dense layer split-K rs_gemm / rs_col_sum
          / rs_prelu_rows_bwd, rs_bn_train_bwd, rs_masked_softmax_pool_bwd,
          rs_din_att_concat_bwd; then one rs_sgd_update_multi over every dense parameter
          and row-sparse rs_embedding_sgd of the behaviour tables (history
          rows, then candidates) and the other sparse tables.
        Dropout(dnn_dropout) after the DNN (:93) runs in training mode: one
        rs_dropout draw on the last DNN output, the same mask regenerated on
        its gradient (dropout=False turns it off, a float overrides the
        rate).  Returns per-sample losses (before the step) if
        ``return_loss``."""
        att, bn = self.att_layer, self.bn_layer
        rate = _dropout_rate(self, dropout)
        dev, st = self._dev, _lib.stream()
        nb = len(self.seq_feats)
        hists = [_ids_tensor(inputs[f["feat"]], dev) for f in self.seq_feats]
        B, T = hists[0].shape
        if any(h.shape != (B, T) for h in hists):
            raise ValueError("DIN: every behaviour feature must be [B, T]")
        cand = _ids_tensor(inputs["movie_id"], dev).reshape(B, -1)
        if cand.shape[1] != nb:
            raise ValueError(f"DIN: inputs['movie_id'] needs one candidate id per behaviour feature ({nb})")
        if self.out_layer.kernel is None:
            self.forward(inputs, check_ids)  # Keras build on the first call
        if T != att.T:
            raise ValueError(f"Attention built for T={att.T} (PReLU alpha is [T,h]); got T={T}")
        labels = _to_device_f32(labels, dev).reshape(-1)
        emp = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
        K = sum(l.k for l in self.embed_seq_layers)
        M = B * T
        width = 2 * K + sum(l.k for l in self.embed_sparse_layers) + self.dense_num
        shapes = [(W.shape[0], W.shape[1], M) for W in att.kernels] + [(att.out_kernel.shape[0], 1, M)]
        shapes += [(L.kernel.shape[0], L.kernel.shape[1], B) for L in self._layers()]
        lb = _lib.lib()
        # one scratch buffer for every stream-ordered call below (gemm split-K
        # slices, column-sum slices, the PReLU backward's products)
        need = [gemm_need(shapes + [(m, kin, n) for kin, n, m in shapes])]  # dW and d_in orientations
        need += [lb.rs_col_sum_workspace_size(m, n) for _, n, m in shapes]
        need += [lb.rs_prelu_rows_bwd_workspace_size(M, W.shape[1], T) for W in att.kernels]
        need += [lb.rs_prelu_rows_bwd_workspace_size(B, L.units, 1) for L in self.dense_layer]
        need += [lb.rs_dice_train_workspace_size(M, 4 * K)] if att.activation == "dice" else []
        need += [lb.rs_dice_train_workspace_size(B, L.units) for L in self.dense_layer if L.activation == "dice"]
        # the PReLU unit with two hidden layers (the reference default (80, 40)):
        # rs_din_att_prelu_bwd when its shape fits; otherwise layer by layer
        att_fused = (self.fused_att_train and att.activation == "prelu" and len(att.kernels) == 2
                     and lb.rs_din_att_prelu_bwd_workspace_size(B, T, 4 * K, *att.kernels[1].shape) >= 0)
        if att_fused:
            need.append(lb.rs_din_att_prelu_bwd_workspace_size(B, T, 4 * K, *att.kernels[1].shape))
        gw = gemm_ws(self, max(need))

        # ---- forward, keeping what the backward needs
        hist_ids = [h.reshape(M, 1) for h in hists]
        cand_ids = [cand[:, i:i + 1] for i in range(nb)]
        item = self._behaviour_embed(cand_ids, B, check_ids)
        seq = self._behaviour_embed(hist_ids, M, check_ids)
        x = emp(B, width)
        h0 = emp(M, 4 * K)
        call("rs_din_att_concat", ptr(item), ptr(seq), B, T, K, ptr(h0), st)
        att_in, att_pre = [h0], []

        def dice_fwd(d, x, m, n):
            # Dice under fit: batch statistics (kept for the backward), moving averages moved
            mu, vr, y = emp(n), emp(n), emp(m, n)
            call("rs_dice_train_fwd", ptr(x), m, n, ptr(d.alphas), d.epsilon, 0.99, ptr(d.moving_mean),
                 ptr(d.moving_variance), ptr(mu), ptr(vr), ptr(y), *gw, st)
            return (mu, vr), y

        score = emp(M)
        if att_fused:  # the unit's forward in one launch, z1 / z2 kept
            (W1, W2), (b1, b2), (al1, al2) = att.kernels, att.biases, att.alphas
            att_pre = [emp(M, W1.shape[1]), emp(M, W2.shape[1])]
            call("rs_din_att_prelu_fwd", ptr(h0), ptr(W1), ptr(b1), ptr(al1), ptr(W2), ptr(b2), ptr(al2),
                 ptr(att.out_kernel), ptr(att.out_bias), B, T, 4 * K, W1.shape[1], W2.shape[1], ptr(att_pre[0]),
                 ptr(att_pre[1]), ptr(score), st)
        else:
            for W, b, al in zip(att.kernels, att.biases, att.alphas):
                n = W.shape[1]
                z, y = emp(M, n), emp(M, n)
                call("rs_dense_fwd", ptr(att_in[-1]), att_in[-1].stride(0), ptr(W), ptr(b), None, _lib.ACT[None],
                     ptr(z), n, M, W.shape[0], n, st)
                call("rs_prelu_rows_fwd", ptr(z), M, n, ptr(al), T, ptr(y), st)
                att_pre.append(z)
                att_in.append(y)
            for d in att.dice:  # att_attention 'dice': Dice layers on the 4k-wide concat, no Dense
                saved, y = dice_fwd(d, att_in[-1], M, 4 * K)
                att_pre.append(saved)
                att_in.append(y)
            hl = att_in[-1]
            call("rs_dense_fwd", ptr(hl), hl.stride(0), ptr(att.out_kernel), ptr(att.out_bias), None,
                 _lib.ACT[None], ptr(score), 1, M, hl.shape[1], 1, st)
        a = emp(B, T)
        h_first = hists[0]
        call("rs_masked_softmax_pool", ptr(score), ptr(h_first), _lib.id_kind(h_first), h_first.stride(0), ptr(seq),
             B, T, K, ptr(a), ptr(x), width, st)
        x[:, K:2 * K].copy_(item)
        col = 2 * K
        other_ids = []
        for f, layer in zip(self.other_sparse, self.embed_sparse_layers):
            ids = _ids_tensor(inputs[f["feat"]], dev).reshape(B, 1)
            other_ids.append(ids)
            layer.gather(ids, out=x[:, col:col + layer.k], check_ids=check_ids)
            col += layer.k
        for f in self.dense_feature_columns:
            x[:, col:col + 1] = _to_device_f32(inputs[f["feat"]], dev).reshape(B, 1)
            col += 1
        bn_saved, y0 = bn_train_fwd(bn, x, st)
        acts, pre, dsaved = [y0], [], []
        for L in self.dense_layer:
            z, y = emp(B, L.units), emp(B, L.units)
            call("rs_dense_fwd", ptr(acts[-1]), acts[-1].stride(0), ptr(L.kernel), ptr(L.bias), None,
                 _lib.ACT[None], ptr(z), L.units, B, L.kernel.shape[0], L.units, st)
            if L.activation == "dice":
                saved, y = dice_fwd(L.dice, z, B, L.units)
                dsaved.append(saved)
            else:
                call("rs_prelu_rows_fwd", ptr(z), B, L.units, ptr(L.alpha), 1, ptr(y), st)
                dsaved.append(None)
            pre.append(z)
            acts.append(y)
        if rate > 0:  # in place: the backward reads the layers' pre-activations, and BN's input, only
            rng = _dropout_rng(self)
            drop_off = rng.draw(acts[-1], rate, st)
        out = self.out_layer
        logit = emp(B)
        call("rs_dense_fwd", ptr(acts[-1]), acts[-1].stride(0), ptr(out.kernel), ptr(out.bias), None,
             _lib.ACT[None], ptr(logit), 1, B, out.kernel.shape[0], 1, st)
        g, loss = bce_head_logit(logit, labels, return_loss, st)

        # ---- backward (every gradient before any update)
        # (every Dense here: column sums on the workspace, rs_col_sum_split; PReLU / Dice below, so no mask)
        updates = []

        def prelu_back(z, dy, alpha, period, m):
            n = z.shape[1]
            dz, dal = emp(m, n), emp(alpha.numel())
            call("rs_prelu_rows_bwd", ptr(z), ptr(dy), m, n, ptr(alpha), period, ptr(dz), ptr(dal), *gw, st)
            updates.append((alpha, dal))
            return dz

        def dice_back(d, x, saved, dy, m, n):
            dx, dal = emp(m, n), emp(n)
            call("rs_dice_train_bwd", ptr(x), m, n, ptr(d.alphas), ptr(saved[0]), ptr(saved[1]), d.epsilon, ptr(dy),
                 ptr(dx), ptr(dal), *gw, st)
            updates.append((d.alphas, dal))
            return dx

        dW, db, dh = dense_backward(out.kernel, acts[-1], g.view(B, 1), gw, emp, st, split_sum=True)
        updates.extend([(out.kernel, dW), (out.bias, db)])
        if rate > 0:
            rng.redraw(dh, rate, drop_off, st)
            rng.end_step(st)
        for li in reversed(range(len(self.dense_layer))):
            L = self.dense_layer[li]
            if L.activation == "dice":
                dz = dice_back(L.dice, pre[li], dsaved[li], dh, B, L.units)
            else:
                dz = prelu_back(pre[li], dh, L.alpha, 1, B)
            dW, db, dh = dense_backward(L.kernel, acts[li], dz, gw, emp, st, split_sum=True)
            updates.extend([(L.kernel, dW), (L.bias, db)])
        dx, dgam, dbet = bn_train_bwd(bn, x, bn_saved, dh, st)
        updates.extend([(bn.gamma, dgam), (bn.beta, dbet)])
        ds, dseq = emp(M), emp(M, K)
        call("rs_masked_softmax_pool_bwd", ptr(a), ptr(h_first), _lib.id_kind(h_first), h_first.stride(0), ptr(seq),
             ptr(dx), width, B, T, K, ptr(ds), ptr(dseq), st)
        if att_fused:
            # the whole attention-unit backward in one launch (+ its partial sums)
            (W1, W2), (b1, b2), (al1, al2) = att.kernels, att.biases, att.alphas
            h1, h2 = W2.shape
            dh3 = emp(M, 4 * K)
            gr = [emp(4 * K, h1), emp(h1), emp(T, h1), emp(h1, h2), emp(h2), emp(T, h2), emp(h2), emp(1)]
            call("rs_din_att_prelu_bwd", ptr(h0), ptr(att_pre[0]), ptr(att_pre[1]), ptr(ds), ptr(W1), ptr(W2),
                 ptr(al1), ptr(al2), ptr(att.out_kernel), B, T, 4 * K, h1, h2, ptr(dh3), *[ptr(v) for v in gr], *gw,
                 st)
            updates.extend(zip([W1, b1, al1, W2, b2, al2, att.out_kernel, att.out_bias], gr))
        else:
            dW, db, dh3 = dense_backward(att.out_kernel, hl, ds.view(M, 1), gw, emp, st, split_sum=True)
            updates.extend([(att.out_kernel, dW), (att.out_bias, db)])
            for li in reversed(range(len(att.kernels))):
                dz = prelu_back(att_pre[li], dh3, att.alphas[li], T, M)
                dW, db, dh3 = dense_backward(att.kernels[li], att_in[li], dz, gw, emp, st, split_sum=True)
                updates.extend([(att.kernels[li], dW), (att.biases[li], db)])
        for li in reversed(range(len(att.dice))):
            dh3 = dice_back(att.dice[li], att_in[li], att_pre[li], dh3, M, 4 * K)
        call("rs_din_att_concat_bwd", ptr(dh3), ptr(item), ptr(seq), B, T, K, ptr(dx) + 4 * K, width, ptr(dseq), st)

        # ---- SGD
        _lib.sgd_update_multi([(w, gr, gr.numel(), 0.0) for w, gr in updates], lr, st)
        col = 0  # (each table is a one-field EmbedLayer; the history's [B*T, 1] ids come first and size _emb_ws)
        for i, layer in enumerate(self.embed_seq_layers):
            embedding_sgd(layer, hist_ids[i], ptr(dseq) + 4 * col, K, lr, st, self)
            embedding_sgd(layer, cand_ids[i], ptr(dx) + 4 * (K + col), width, lr, st, self)
            col += layer.k
        col = 2 * K
        for layer, ids in zip(self.embed_sparse_layers, other_ids):
            embedding_sgd(layer, ids, ptr(dx) + 4 * col, width, lr, st, self)
            col += layer.k
        self._weights_changed()
        for L in list(self.embed_seq_layers) + list(self.embed_sparse_layers):
            L._weights_changed()
        return loss


# ------------------------------------ other CTR models
class NFM(TowerMixin, KerasModule):
    """NFM(feature_columns, hidden_units, output_dim, activation='relu',
    dropout=0) — model/nfm.py:13-33, with 3-D embeddings (documented
    deviation: on the reference's rank-2 EmbedLayer output the bi-interaction
    reduce_sum collapses to [B] and the concat with the dense block fails):
    x = BN(concat([dense, 0.5((sum_f e)^2 - sum_f e^2)])) -> DNNLayer ->
    Dense(1) -> sigmoid.  ids -> rows -> bi-interaction -> [dense | pooled]
    in one launch (rs_embed_pair_pool_fwd), BN (rs_affine_act), then the
    DNNLayer + output Dense as ONE tower launch (rs_mlp_fwd)."""

    def __init__(self, feature_columns, hidden_units, output_dim, activation="relu", dropout=0, embed_dim=8,
                 device=None, seed=None):
        super().__init__(device, seed)
        self.dense_feature_columns, self.sparse_feature_columns = feature_columns
        self.nd = len(self.dense_feature_columns)
        self.dnn_layers = DNNLayer(hidden_units, output_dim, activation, dropout, device=device,
                                   seed=_subseed(self._gen))
        self.emb_layers = EmbedLayer(self.sparse_feature_columns, embed_dim, device=device, seed=_subseed(self._gen))
        self.bn_layer = BatchNormalization(device=device)
        self.output_layer = Dense(1, activation="sigmoid", device=device, seed=_subseed(self._gen))
        d = self.nd + embed_dim
        self.dnn_layers.build(d)
        self.output_layer.build(int(output_dim))
        self.bn_layer.build(d)
        self._err = _ErrFlag(self._dev)

    def _layers(self):
        return list(self.dnn_layers.hidden_layer) + [self.dnn_layers.output_layer, self.output_layer]

    def bi_interaction_input(self, inputs, check_ids=True):
        """concat([dense, BiInteraction(emb)]) [B, nd+k] (model/nfm.py:26-29)."""
        dense, ids = _split_criteo(inputs, self.nd, self._dev)
        e = self.emb_layers
        B = ids.shape[0]
        x = torch.empty(B, self.nd + e.k, dtype=torch.float32, device=self._dev)
        call("rs_embed_pair_pool_fwd", ptr(ids), _lib.id_kind(ids), ids.stride(0), ptr(e.table),
             ptr(e.field_offsets), ptr(e.field_vocab), e.n_fields, e.k, 0, ptr(dense), dense.stride(0), self.nd,
             ptr(x), x.stride(0), self.nd, None, None, 0, None, B, ptr(self._err.t), _lib.stream())
        if check_ids:
            self._err.check("NFM")
        return x

    def forward(self, inputs, check_ids=True):
        x = self.bi_interaction_input(inputs, check_ids)
        if self.tower_ok():
            # BatchNormalization + DNNLayer + Dense(1, sigmoid) in one launch
            if self.bn_layer.gamma is None:
                self.bn_layer.build(x.shape[-1])
            return self.tower(x, in_affine=self.bn_layer.affine())
        return self.output_layer(self.dnn_layers(self.bn_layer(x)))

    def train_step(self, inputs, labels, lr=0.01, return_loss=False, check_ids=True, dropout=None):
        """One step of compile_fit on NFM (utils/compile_fit.py:9-15; the
        reference's NFM demo trains this way, model/nfm.py:47) with
        NFM.call in training mode:
          [dense | Bi-Interaction] (rs_embed_pair_pool_fwd) and the rows
          (rs_embed_gather), rs_bn_train_fwd (batch statistics, moving
          averages), the DNNLayer + output Dense with saved activations
          (rs_dense_fwd, logit), rs_head_grad, the DNN backward (rs_gemm /
          rs_col_sum), rs_bn_train_bwd, rs_bi_interaction_bwd (de_f = dbi
          (S - e_f)), SGD of the dense parameters and row-sparse
          rs_embedding_sgd.  DNNLayer's Dropout after each hidden layer
          (layer/interaction.py:44) runs in training mode as in
          DeepFM.train_step (counter-based rs_dropout masks, regenerated in
          the backward; dropout=False turns it off, a float overrides the rate).
        Returns per-sample losses (before the step) if ``return_loss``."""
        dnn = self.dnn_layers
        rate = _dropout_rate(dnn, dropout)
        _check_train_tower("NFM", dnn)
        dense, ids = _split_criteo(inputs, self.nd, self._dev)
        labels = _to_device_f32(labels, self._dev).reshape(-1)
        e, bn, out = self.emb_layers, self.bn_layer, self.output_layer
        B, F, k, st, dev = ids.shape[0], e.n_fields, e.k, _lib.stream(), self._dev
        emp = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
        x = self.bi_interaction_input(inputs, check_ids)  # [B, nd + k]
        rows = e.gather(ids, check_ids=False)             # [B, F*k] (ids checked above)
        D = self.nd + k
        bn_saved, y0 = bn_train_fwd(bn, x, st)
        layers = self._layers()
        acts, drop = _dnn_train_forward(self, dnn, y0, rate, st)
        acts.append(dnn.output_layer(acts[-1]))
        logit = emp(B)
        call("rs_dense_fwd", ptr(acts[-1]), acts[-1].stride(0), ptr(out.kernel), ptr(out.bias), None,
             _lib.ACT[None], ptr(logit), 1, B, out.kernel.shape[0], 1, st)
        g, loss = bce_head_logit(logit, labels, return_loss, st)
        gw = gemm_ws(self, gemm_need([(*L.kernel.shape, B) for L in layers]))
        grads, delta = _dnn_backward(layers, acts, g.view(B, 1), gw, emp, st, drop=drop)
        dx, dgam, dbet = bn_train_bwd(bn, x, bn_saved, delta, st)
        de = emp(B, F * k)
        call("rs_bi_interaction_bwd", ptr(rows), F * k, ptr(dx) + 4 * self.nd, D, F, k, B, ptr(de), F * k, st)
        _lib.sgd_update_multi(_dnn_updates(grads) + [(bn.gamma, dgam, D, 0.0), (bn.beta, dbet, D, 0.0)], lr, st)
        embedding_sgd(e, ids, ptr(de), F * k, lr, st, self)
        self._weights_changed()
        return loss


class AFM(KerasModule):
    """AFM(feature_columns, mode) — model/afm.py:11-19: sigmoid(AFMLayer(x)),
    i.e. sigmoid(sigmoid(Dense(1)(pool over pairs))) — both sigmoids in the
    one rs_embed_pair_pool_fwd launch."""

    def __init__(self, feature_columns, mode, device=None, seed=None):
        super().__init__(device, seed)
        self.afm_layer = AFMLayer(feature_columns, mode, device=device, seed=_subseed(self._gen))

    def forward(self, inputs, check_ids=True):
        return self.afm_layer.pooled(inputs, check_ids, n_sigmoid=2)[1]

    def train_step(self, inputs, labels, lr=0.01, return_loss=False, check_ids=True):
        """One step of compile_fit on AFM (utils/compile_fit.py:9-15 on
        model/afm.py:15-18): BCE on the input of AFM.call's second sigmoid
        (Keras takes it as the logit), plain SGD, no regulariser.
          rs_afm_train_fwd: ids -> rows -> pooled pairs -> Dense(1) -> both
          sigmoids -> g = dL/d(Dense output) -> dL/d(row) of every looked-up
          row, one launch; the id check (``check_ids``: it raises before any
          weight changes); dW = pooled^T g (rs_gemm) and db = sum g
          (rs_col_sum); one rs_sgd_update_multi for the Dense(1); row-sparse
          rs_embedding_sgd.
        'att' pools by the sum (AttentionLayer's softmax runs over a size-1
        axis), so attention_w / attention_h get an exactly zero gradient and
        stay as they are.  'max' sends a tie's gradient to the first tied pair
        in row-major order (TF splits it evenly).  ``inputs`` as in forward.
        Returns the per-sample losses before the step if ``return_loss``."""
        if self._dev.type != "cuda":
            raise NotImplementedError("AFM.train_step: training runs only on a HIP device")
        layer = self.afm_layer
        if isinstance(inputs, (tuple, list)):
            ids = _ids_tensor(inputs[1], self._dev)
        else:
            ids = _to_device_f32(inputs, self._dev)[:, layer.nd:]
        labels = _to_device_f32(labels, self._dev).reshape(-1)
        e, head = layer.embed_layer, layer.output_layer
        B, F, k, st = ids.shape[0], e.n_fields, layer.k, _lib.stream()
        emp = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=self._dev)
        pooled, g, de = emp(B, k), emp(B), emp(B, F * k)
        loss = emp(B) if return_loss else None
        call("rs_afm_train_fwd", ptr(ids), _lib.id_kind(ids), ids.stride(0), ptr(e.table), ptr(e.field_offsets),
             ptr(e.field_vocab), F, k, _AFM_MODES.get(layer.mode, 0), ptr(head.kernel), ptr(head.bias), 2,
             ptr(labels), B, ptr(pooled), k, None, ptr(g), ptr(loss), ptr(de), F * k, ptr(layer._err.t), st)
        if check_ids:
            layer._err.check("AFM.train_step")
        gw = gemm_ws(self, gemm_need([(k, 1, B)]))
        dW, db, _ = dense_backward(head.kernel, pooled, g.view(B, 1), gw, emp, st, d_in=False)
        _lib.sgd_update_multi([(head.kernel, dW, k, 0.0), (head.bias, db, 1, 0.0)], lr, st)
        embedding_sgd(e, ids, ptr(de), F * k, lr, st, self)
        self._weights_changed()
        return loss


class FFM(KerasModule):
    """FFM(feature_columns, k, w_reg=1e-4, v_reg=1e-4) — model/ffm.py:10-22:
    sigmoid(FFMLayer(x)), one launch (rs_ffm_fwd)."""

    def __init__(self, feature_columns, k, w_reg=1e-4, v_reg=1e-4, device=None, seed=None):
        super().__init__(device, seed)
        self.dense_feature_columns, self.sparse_feature_columns = feature_columns
        self.ffm = FFMLayer(feature_columns, k, w_reg, v_reg, device=device, seed=_subseed(self._gen))

    def forward(self, inputs):
        return self.ffm.logits(inputs, n_sigmoid=1)

    def train_step(self, inputs, labels, lr=0.01, return_loss=False):
        """One step of compile_fit on FFM (utils/compile_fit.py:9-15; the
        reference's FFM demo trains this way, model/ffm.py:36): BCE on
        sigmoid(FFMLayer) plus FFMLayer's l2(w_reg) / l2(v_reg) regularisers on
        every row of w / v (layer/interaction.py:131-139), plain SGD:
          rs_ffm_train_fwd (per sample: Fm, z, g and the shared gradient row
          G = g (T - Fm)), rs_gemm / rs_col_sum (the dense rows' and w0's
          gradients), rs_l2_decay (every row of w and v), rs_sgd_update_multi (dense
          rows, w0) and rs_embedding_sgd_strided (each looked-up row of v
          gets its sample's G, of w its g; duplicates summed in lookup order).
        Out-of-range ids train nothing (tf.one_hot's zero row).  Every
        gradient comes from the pre-step weights.  Returns per-sample losses
        (before the step) if ``return_loss``."""
        L = self.ffm
        dense, ids = _split_criteo(inputs, L.nd, self._dev)
        labels = _to_device_f32(labels, self._dev).reshape(-1)
        B, F, k, nd, st, dev = ids.shape[0], len(L.onehot_dims), L.k, L.nd, _lib.stream(), self._dev
        E = L.field_num * k
        emp = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
        G, g = emp(B, E), emp(B)
        loss = emp(B) if return_loss else None
        call("rs_ffm_train_fwd", ptr(ids), _lib.id_kind(ids), ids.stride(0), ptr(dense), dense.stride(0), nd,
             ptr(L.v), ptr(L.w), ptr(L.w0), ptr(L.field_offsets), ptr(L.field_vocab), F, k, ptr(labels), B, ptr(G),
             ptr(g), ptr(loss), st)
        gw = gemm_ws(self, gemm_need([(nd, E, B), (nd, 1, B)]))
        dvd, dwd, dw0 = emp(max(nd, 1), E), emp(max(nd, 1)), emp(1)
        if nd:
            call("rs_gemm", 1, 0, nd, E, B, 1.0, ptr(dense), dense.stride(0), ptr(G), E, 0.0, ptr(dvd), E, None, 0,
                 *gw, st)
            call("rs_gemm", 1, 0, nd, 1, B, 1.0, ptr(dense), dense.stride(0), ptr(g), 1, 0.0, ptr(dwd), 1, None, 0,
                 *gw, st)
        call("rs_col_sum", ptr(g), 1, B, 1, ptr(dw0), st)
        # l2 on every row (old weights), then the data gradients
        call("rs_l2_decay", ptr(L.v), L.v.numel(), float(lr), float(L.v_reg), st)
        call("rs_l2_decay", ptr(L.w), L.w.numel(), float(lr), float(L.w_reg), st)
        _lib.sgd_update_multi(([(L.v, dvd, nd * E, 0.0), (L.w, dwd, nd, 0.0)] if nd else []) + [(L.w0, dw0, 1, 0.0)],
                              lr, st)
        n_sparse = L.feature_num - nd
        embedding_sgd_strided(ptr(L.v) + 4 * nd * E, n_sparse, E, ids, L.field_offsets, L.field_vocab, G, lr, st, self)
        embedding_sgd_strided(ptr(L.w) + 4 * nd, n_sparse, 1, ids, L.field_offsets, L.field_vocab, g, lr, st, self)
        self._weights_changed()
        return loss


def _prefixed(prefix, weights):
    return {f"{prefix}/{k}": v for k, v in weights.items()}


def _set_prefixed(module, prefix, weights, strict):
    """module.set_keras_weights on the entries of `weights` under prefix/."""
    own = {k[len(prefix) + 1:]: v for k, v in weights.items() if k.startswith(prefix + "/")}
    if not strict:
        own = {k: v for k, v in own.items() if k in module.keras_weights()}
    if strict:
        missing = set(module.keras_weights()) - set(own)
        if missing:
            raise KeyError(f"missing weights {sorted(prefix + '/' + m for m in missing)}")
    if own or strict:
        module.set_keras_weights(own, strict)


class DeepCrossing(KerasModule):
    """DeepCrossing(feature_columns, k, hidden_units, res_layer_num) —
    model/deepCrossing.py:15-32: x = [dense | EmbedLayer(sparse)] through
    res_layer_num ResLayers (each with its own weights; one ``hidden_units``
    serves them all, so units of differing shapes cannot occur), then
    Dense(1, sigmoid).

    ``k`` is accepted and ignored, as in the reference (its EmbedLayer keeps
    the default width 8); the embedding width is ``embed_dim``.

    ``forward_fused`` is ONE launch from the ids (rs_deepcrossing_fwd: the
    concat is never written, every activation stays in LDS);
    ``forward_unfused`` is the gather, one launch per unit (or the per-layer
    composition where the tower kernel does not take the shape), then the
    Dense + sigmoid.  ``forward`` takes the fused path when ``fused_ok()``.
    ``train_step`` is one step of compile_fit (model/deepCrossing.py:45)."""

    def __init__(self, feature_columns, k, hidden_units, res_layer_num, embed_dim=8, device=None, seed=None):
        super().__init__(device, seed)
        self.dense_feature_columns, self.sparse_feature_columns = feature_columns
        self.nd = len(self.dense_feature_columns)
        self.k = k  # unused, as in the reference
        self.hidden_units = [int(u) for u in hidden_units]
        self.embed_layer = EmbedLayer(self.sparse_feature_columns, embed_dim, device=device, seed=_subseed(self._gen))
        self.d = self.nd + self.embed_layer.n_fields * self.embed_layer.k
        self.res_layer = torch.nn.ModuleList(
            [ResLayer(self.hidden_units, device=device, seed=_subseed(self._gen)) for _ in range(int(res_layer_num))])
        for unit in self.res_layer:
            unit.build(self.d)
        self.output_layer = Dense(1, activation="sigmoid", device=device, seed=_subseed(self._gen), input_dim=self.d)
        self._err = _ErrFlag(self._dev)

    def keras_weights(self):
        out = _prefixed("embed_layer", self.embed_layer.keras_weights())
        for u, unit in enumerate(self.res_layer):
            out.update(_prefixed(f"res_layer_{u}", unit.keras_weights()))
        out.update(_prefixed("output_layer", self.output_layer.keras_weights()))
        return out

    def set_keras_weights(self, weights, strict=True):
        if strict:
            unknown = set(weights) - set(self.keras_weights())
            if unknown:
                raise KeyError(f"unknown weights {sorted(unknown)}")
        _set_prefixed(self.embed_layer, "embed_layer", weights, strict)
        for u, unit in enumerate(self.res_layer):
            _set_prefixed(unit, f"res_layer_{u}", weights, strict)
        _set_prefixed(self.output_layer, "output_layer", weights, strict)
        self._weights_changed()

    def _all_layers(self):
        return [l for unit in self.res_layer for l in unit._layers()] + [self.output_layer]

    def fused_ok(self):
        n = len(self.res_layer)
        return (1 <= n <= _RES_MAXU and 1 <= len(self.hidden_units) <= _RES_MAXH
                and self.embed_layer.n_fields >= 1 and self.embed_layer.table.data_ptr() % 16 == 0
                and _res_ok(self.d, self.hidden_units, n))

    def prepared(self):
        """Every unit's weights and the head packed for rs_deepcrossing_fwd,
        cached until a weight changes."""
        return self._packed("res", _res_params(self._all_layers()),
                            lambda: _res_prepare(list(self.res_layer), self.output_layer, self._dev))

    def forward_fused(self, inputs, check_ids=True, x_last=None):
        """DeepCrossing.call as ONE kernel (rs_deepcrossing_fwd).  x_last
        (optional, [B, d]) receives the last unit's output."""
        dense, ids = _split_criteo(inputs, self.nd, self._dev)
        B = ids.shape[0]
        e = self.embed_layer
        nh = len(self.hidden_units)
        out = torch.empty(B, 1, dtype=torch.float32, device=self._dev)
        call("rs_deepcrossing_fwd", ptr(ids), _lib.id_kind(ids), ids.stride(0), ptr(dense) if self.nd else None,
             dense.stride(0) if self.nd else 0, self.nd, ptr(e.table), ptr(e.field_offsets), ptr(e.field_vocab),
             e.n_fields, e.k, nh, ints(self.hidden_units), len(self.res_layer), ptr(self.prepared()),
             ptr(out), ptr(x_last), 0 if x_last is None else x_last.stride(0), B, ptr(self._err.t), _lib.stream())
        if check_ids:
            self._err.check("DeepCrossing")
        return out

    def forward_unfused(self, inputs, check_ids=True):
        """rs_embed_gather, one ResLayer forward per unit, Dense(1, sigmoid)."""
        dense, ids = _split_criteo(inputs, self.nd, self._dev)
        x = self.embed_layer.gather(ids, dense if self.nd else None, check_ids=check_ids)
        for unit in self.res_layer:
            x = unit(x)
        return self.output_layer(x)

    def forward(self, inputs, check_ids=True):
        if self.fused_ok():
            return self.forward_fused(inputs, check_ids)
        return self.forward_unfused(inputs, check_ids)

    def prepared_bwd(self):
        """The backward weight image (rs_res_tower_prepare_bwd: every unit's
        kernels transposed, last unit first, and the head's kernel), cached
        under the key of ``prepared``."""
        def build():
            nh, nu = len(self.hidden_units), len(self.res_layer)
            ci = ints(self.hidden_units)
            img = sized("rs_res_tower_bwd_prepared_size", self.d, nh, ci, nu, device=self._dev)
            call("rs_res_tower_prepare_bwd", self.d, nh, ci, nu, ptrs([l.kernel for l in self._all_layers()[:-1]]),
                 ptr(self.output_layer.kernel), ptr(img), _lib.stream())
            return img
        return self._packed("res_bwd", _res_params(self._all_layers()), build)

    def train_step(self, inputs, labels, lr=0.01, return_loss=False, check_ids=True, fused=None):
        """One step of compile_fit (utils/compile_fit.py:9-15: SGD(lr), binary
        cross-entropy on the sigmoid head; model/deepCrossing.py:45 — the model
        has no regulariser, Dropout or BN), every weight updated in place.

        ``fused=True``: the forward with saved activations from the ids in one
        launch (rs_deepcrossing_train_fwd), rs_head_grad, the whole backward
        data path in one launch (rs_res_tower_bwd: every layer's delta and
        dL/dx_0).  ``fused=False``: rs_embed_gather, rs_dense_fwd per layer
        with a torch add / relu per unit, and _dnn_backward per unit with a
        torch mask / add at the joins.  Both then take the weight gradients
        from the same deterministic blocks (rs_gemm(trans_a) + rs_col_sum per
        layer), one rs_sgd_update_multi and the row-sparse rs_embedding_sgd.
        ``None`` picks fused when ``fused_ok()``; ``True`` raises where the
        kernels do not take the shape.  A bad id raises IndexError before any
        weight changes (``check_ids``).  Returns the per-sample losses before
        the step if ``return_loss``."""
        if self._dev.type != "cuda":
            raise NotImplementedError("DeepCrossing.train_step: training runs only on a HIP device")
        if fused is None:
            fused = self.fused_ok()
        elif fused and not self.fused_ok():
            raise ValueError("DeepCrossing.train_step(fused=True): the residual tower kernels do not take this shape")
        dense, ids = _split_criteo(inputs, self.nd, self._dev)
        labels = _to_device_f32(labels, self._dev).reshape(-1)
        e, head = self.embed_layer, self.output_layer
        units = [u._layers() for u in self.res_layer]
        B, d, st, dev = ids.shape[0], self.d, _lib.stream(), self._dev
        nh, nu = len(self.hidden_units), len(units)
        emp = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
        all_layers = self._all_layers()
        gw = gemm_ws(self, gemm_need([(*L.kernel.shape, B) for L in all_layers]))
        if fused:
            ci = ints(self.hidden_units)
            widths = self.hidden_units + [d]
            saved = emp(B * (d + nu * sum(widths)))
            deltas = emp(B * nu * sum(widths))
            prob, logit, dx0 = emp(B), emp(B), emp(B, d)
            call("rs_deepcrossing_train_fwd", ptr(ids), _lib.id_kind(ids), ids.stride(0),
                 ptr(dense) if self.nd else None, dense.stride(0) if self.nd else 0, self.nd, ptr(e.table),
                 ptr(e.field_offsets), ptr(e.field_vocab), e.n_fields, e.k, nh, ci, nu, ptr(self.prepared()),
                 ptr(saved), ptr(prob), ptr(logit), B, ptr(self._err.t), st)
            if check_ids:
                self._err.check("DeepCrossing.train_step")
            g, loss = bce_head_logit(logit, labels, return_loss, st)
            call("rs_res_tower_bwd", ptr(saved), d, nh, ci, nu, ptr(self.prepared_bwd()), None, 0, ptr(g),
                 ptr(deltas), ptr(dx0), d, B, st)
            # views of saved / deltas: x_u and a_{u,l}, delta_{u,l}
            xs, acts, dels, so, do = [saved[:B * d].view(B, d)], [], [], B * d, 0
            for u in range(nu):
                au, du = [], []
                for n in widths:
                    au.append(saved[so:so + B * n].view(B, n))
                    du.append(deltas[do:do + B * n].view(B, n))
                    so, do = so + B * n, do + B * n
                acts.append(au)
                dels.append(du)
                xs.append(au[-1])
            grads = []
            for u, layers in enumerate(units):
                for l, L in enumerate(layers):
                    a_in = xs[u] if l == 0 else acts[u][l - 1]
                    dW, db, _ = dense_backward(L.kernel, a_in, dels[u][l], gw, emp, st, d_in=False)
                    grads.append((L, dW, db))
            dWh, dbh, _ = dense_backward(head.kernel, xs[nu], g.view(B, 1), gw, emp, st, d_in=False)
            grads.append((head, dWh, dbh))
        else:
            x = e.gather(ids, dense if self.nd else None, check_ids=check_ids)
            xs, acts = [x], []
            for layers in units:
                au = [xs[-1]]
                for L in layers[:-1]:
                    au.append(L(au[-1]))
                xs.append(torch.relu(xs[-1] + layers[-1](au[-1])))
                acts.append(au)
            logit = emp(B)
            call("rs_dense_fwd", ptr(xs[-1]), xs[-1].stride(0), ptr(head.kernel), ptr(head.bias), None, _lib.ACT[None],
                 ptr(logit), 1, B, d, 1, st)
            g, loss = bce_head_logit(logit, labels, return_loss, st)
            grads, dy = _dnn_backward([head], [xs[-1]], g.view(B, 1), gw, emp, st)
            for u in reversed(range(nu)):
                eu = dy * (xs[u + 1] > 0)
                gu, below = _dnn_backward(units[u], acts[u], eu, gw, emp, st)
                grads = gu + grads
                dy = eu + below
            dx0 = dy
        _dnn_apply(grads, lr, st)
        embedding_sgd(e, ids, ptr(dx0) + 4 * self.nd, dx0.stride(0), lr, st, self)
        self._weights_changed()
        return loss


def _packed_f32(x, device):
    """The reference's packed matrix (dtype object / float64 from
    create_criteo_dataset) as a device fp32 tensor (Keras' input autocast)."""
    if not torch.is_tensor(x):
        import numpy as np
        x = np.asarray(x)
        if x.dtype == object:
            x = x.astype(np.float64)
    return _to_device_f32(x, device)


class WideDeep(KerasModule):
    """WideDeep(feature_columns, hidden_units, output_dim, activation) —
    model/wideDeep.py:14-34: sigmoid(0.5 * (WideLayer([dense | one-hot part])
    + DNNLayer(EmbedLayer(sparse)))); the deep input is the embeddings only.

    ``forward(X)`` takes the reference's packed row from
    create_criteo_dataset('WideDeep'): [dense nd | label codes F | dense nd
    again | dummies W] (get_dummies keeps the numeric columns, so the wide
    input [X[:, :nd] | X[:, nd+F:]] holds the dense block twice).
    ``forward_onehot(dense, ids, field_offsets, field_widths)`` takes the
    compact form (dummies column of field c's code: field_offsets[c] + code)
    and gathers the wide weights (rs_wide_onehot_fwd).  The wide weight w is
    built on first use from the input width 2 nd + sum(widths).  With
    output_dim == 1 the deep tower and the head are one rs_mlp_fwd launch;
    otherwise the reference's broadcast [B,1] + [B,output_dim] applies.
    ``train_step(X, labels)`` / ``train_step_onehot(dense, ids, field_offsets,
    field_widths, labels)`` are one step of compile_fit (model/wideDeep.py:47)
    on either form; ``w_reg`` is WideLayer's l2 factor on w."""

    def __init__(self, feature_columns, hidden_units, output_dim, activation, embed_dim=8, device=None, seed=None,
                 w_reg=1e-4):
        super().__init__(device, seed)
        self.dense_feature_columns, self.sparse_feature_columns = feature_columns
        self.nd = len(self.dense_feature_columns)
        self.embed_layer = EmbedLayer(self.sparse_feature_columns, embed_dim, device=device, seed=_subseed(self._gen))
        self.wide = WideLayer(device=device, seed=_subseed(self._gen), w_reg=w_reg)
        self.deep = DNNLayer(hidden_units, output_dim, activation, device=device, seed=_subseed(self._gen))
        self.deep.build(self.embed_layer.n_fields * self.embed_layer.k)
        self.output_dim = int(output_dim)

    def build(self, wide_width):
        """Build the wide weights for a wide input of `wide_width` columns."""
        self.wide.build(wide_width)

    def keras_weights(self):
        out = _prefixed("embed_layer", self.embed_layer.keras_weights())
        out.update(_prefixed("wide", self.wide.keras_weights()))
        out.update(_prefixed("deep", self.deep.keras_weights()))
        return out

    def set_keras_weights(self, weights, strict=True):
        if not self.wide.built and "wide/w" in weights:
            self.wide.build(torch.as_tensor(weights["wide/w"]).shape[0])
        if strict:
            unknown = set(weights) - set(self.keras_weights())
            if unknown:
                raise KeyError(f"unknown weights {sorted(unknown)}")
        _set_prefixed(self.embed_layer, "embed_layer", weights, strict)
        _set_prefixed(self.wide, "wide", weights, strict)
        _set_prefixed(self.deep, "deep", weights, strict)
        self._weights_changed()

    def _combine(self, wide, ids, check_ids):
        emb = self.embed_layer.gather(ids, check_ids=check_ids)
        if self.output_dim == 1 and self.deep.tower_ok():
            return self.deep.tower(emb, extra=wide, c0=0.5, c1=0.5, head=True)
        deep = self.deep(emb)
        return sigmoid_combine(wide.expand(-1, deep.shape[1]).contiguous(), deep, 0.5, 0.5)

    def forward(self, inputs, check_ids=True):
        X = _packed_f32(inputs, self._dev)
        nd, F = self.nd, self.embed_layer.n_fields
        if X.dim() != 2 or X.shape[1] <= nd + F:
            raise ValueError(f"WideDeep: packed input needs more than {nd + F} columns "
                             "([dense | codes | dense | dummies])")
        wide_in = torch.cat([X[:, :nd], X[:, nd + F:]], dim=1)
        return self._combine(self.wide(wide_in), X[:, nd:nd + F], check_ids)

    def forward_onehot(self, dense, ids, field_offsets, field_widths, check_ids=True):
        ids = _ids_tensor(ids, self._dev)
        wide = self.wide.forward_onehot(dense if self.nd else None, ids, field_offsets, field_widths, check_ids)
        return self._combine(wide, ids, check_ids)

    def _train(self, wide, wide_update, ids, labels, lr, return_loss, check_ids, dropout):
        """The step both input forms share: the deep tower forward with saved
        activations on the embedding rows, rs_head_grad on z = 0.5 wide + 0.5
        deep, the tower backward, then ``wide_update(g_wide)`` -> the wide
        part's [(w, grad, n, l2)] entries (and its own launches), one
        rs_sgd_update_multi and the row-sparse rs_embedding_sgd."""
        deep, e = self.deep, self.embed_layer
        layers = deep._layers()
        rate = _dropout_rate(deep, dropout)
        B, st, dev = ids.shape[0], _lib.stream(), self._dev
        emp = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
        emb = e.gather(ids, check_ids=check_ids)  # [B, F*k]: the deep input has no dense block
        acts, drop = _dnn_train_forward(self, deep, emb, rate, st)
        deep_out = deep.output_layer(acts[-1])
        g_w, g_d, loss = bce_head(wide, deep_out, labels, 0.5, 0.5, return_loss, st)
        n = self.wide.w.shape[0]
        gw = gemm_ws(self, gemm_need([(*L.kernel.shape, B) for L in layers] + [(n, 1, B)]))
        grads, demb = _dnn_backward(layers, acts, g_d.view(B, 1), gw, emp, st, drop=drop)
        dw0 = emp(1)
        call("rs_col_sum", ptr(g_w), 1, B, 1, ptr(dw0), st)
        # updates (every gradient above and in wide_update comes from the pre-step weights)
        _lib.sgd_update_multi(_dnn_updates(grads) + wide_update(g_w, gw, emp, st) + [(self.wide.w0, dw0, 1, 0.0)],
                              lr, st)
        embedding_sgd(e, ids, ptr(demb), e.n_fields * e.k, lr, st, self)
        self._weights_changed()
        return loss

    def _check_train(self, what):
        if self._dev.type != "cuda":
            raise NotImplementedError(f"WideDeep.{what}: training runs only on a HIP device")
        if self.output_dim != 1:
            raise NotImplementedError(f"WideDeep.{what}: output_dim 1 only")
        _check_train_tower("WideDeep", self.deep)

    def train_step(self, X, labels, lr=0.01, return_loss=False, check_ids=True, dropout=None):
        """One step of compile_fit (utils/compile_fit.py:9-15; model/wideDeep.py:47)
        on the packed row [dense | codes | dense | dummies]: BCE on sigmoid(0.5
        (wide + deep)), WideLayer's l2(w_reg) on every element of w, plain SGD,
        DNNLayer's Dropout active as in DeepFM.train_step.  The wide part: dw =
        wide_in^T g (rs_gemm), dw0 = sum g (rs_col_sum), the l2 term through
        rs_sgd_update_multi's per-tensor l2.  output_dim 1 and 'relu' / linear
        towers only.  Returns the per-sample losses before the step if
        ``return_loss``."""
        self._check_train("train_step")
        Xd = _packed_f32(X, self._dev)
        nd, F = self.nd, self.embed_layer.n_fields
        if Xd.dim() != 2 or Xd.shape[1] <= nd + F:
            raise ValueError(f"WideDeep: packed input needs more than {nd + F} columns "
                             "([dense | codes | dense | dummies])")
        labels = _to_device_f32(labels, self._dev).reshape(-1)
        wide_in = torch.cat([Xd[:, :nd], Xd[:, nd + F:]], dim=1)
        B, n = wide_in.shape
        wide = self.wide(wide_in)

        def wide_update(g, gw, emp, st):
            dw = emp(n, 1)
            call("rs_gemm", 1, 0, n, 1, B, 1.0, ptr(wide_in), n, ptr(g), 1, 0.0, ptr(dw), 1, None, 0, *gw, st)
            return [(self.wide.w, dw, n, self.wide.w_reg)]

        return self._train(wide, wide_update, Xd[:, nd:nd + F], labels, lr, return_loss, check_ids,
                           dropout)

    def train_step_onehot(self, dense, ids, field_offsets, field_widths, labels, lr=0.01, return_loss=False,
                          check_ids=True, dropout=None):
        """``train_step`` on the compact form (forward_onehot's arguments): no
        one-hot matrix is formed.  The l2 term is rs_l2_decay over all of w
        (from the pre-step weights), the two dense halves of w each get
        dense^T g, and the one-hot rows go through rs_embedding_sgd_strided
        with k = 1 (each looked-up scalar of w gets its sample's g, duplicates
        summed in lookup order)."""
        self._check_train("train_step_onehot")
        dev, nd = self._dev, self.nd
        ids = _ids_tensor(ids, dev)
        dense = _to_device_f32(dense, dev) if nd else None
        labels = _to_device_f32(labels, dev).reshape(-1)
        offs = torch.as_tensor(field_offsets, dtype=torch.int64).to(dev)
        wid = torch.as_tensor(field_widths, dtype=torch.int64).to(dev)
        B, F = ids.shape
        wide = self.wide.forward_onehot(dense, ids, offs, wid, check_ids)
        w = self.wide.w
        n = w.shape[0]

        def wide_update(g, gw, emp, st):
            ups = []
            if nd:
                dwd = emp(nd, 1)
                call("rs_gemm", 1, 0, nd, 1, B, 1.0, ptr(dense), dense.stride(0), ptr(g), 1, 0.0, ptr(dwd), 1, None, 0,
                     *gw, st)
                ups = [(ptr(w), dwd, nd, 0.0), (ptr(w) + 4 * nd, dwd, nd, 0.0)]
            call("rs_l2_decay", ptr(w), n, float(lr), float(self.wide.w_reg), st)
            embedding_sgd_strided(ptr(w) + 4 * 2 * nd, n - 2 * nd, 1, ids, offs, wid, g, lr, st, self, "_wide_ws")
            return ups

        return self._train(wide, wide_update, ids, labels, lr, return_loss, check_ids, dropout)


class _FnnRest(TowerMixin, KerasModule):
    """Layers 2..L + the output Dense of FNN's DNNLayer as a tower of their
    own (their rs_mlp_prepare image: the first layer is the gather)."""

    def __init__(self, dnn):
        super().__init__(dnn._dev)
        self.__dict__["_dnn"] = dnn  # not a submodule: the DNNLayer owns the weights

    def _layers(self):
        return self._dnn._layers()[1:]

    def tower_ok(self):
        return bool(self._layers()) and super().tower_ok()


class FNN(KerasModule):
    """FNN(k, hidden_units, output_dim=1, activation='relu', w_reg=1e-4,
    v_reg=1e-4, dropout=0.2) — the two models of model/fnn.py:13-32 in one
    class: ``self.fm = FM(k, w_reg, v_reg)`` and ``self.dnn =
    DNNLayer(hidden_units, output_dim, activation)`` on x (.) v reshaped to
    [B, n*k] (model/fnn.py:51-57), closed by a sigmoid.  (The reference's
    class name DNN is DIEN's DNN layer here.)

    The dense [B, n*k] input is never formed on the compact path: with the
    first Dense kernel W1 (n*k, H1) viewed as [n, k, H1], z1 = b1 + sum over
    a sample's nd + F active features of x_a * (v[f_a] @ W1[f_a]).
    ``forward_onehot(dense, ids, field_offsets, field_vocab)`` gathers rows of
    the projected table P[f] = v[f] @ W1[f] (rs_fnn_project, cached until a
    weight moves) — in one launch with the rest of the tower where
    ``fused_ok()`` (rs_fnn_fwd), else rs_fnn_first_layer_fwd + the tower
    (``forward_unfused``).  ``forward(X)`` takes the literal one-hot matrix
    [B, n] and forms x (.) v as the reference does (small n only).

    Training follows the script: ``train_step_fm`` is FM.train_step (stage 1),
    ``train_step`` one SGD step of the DNN on the constant x (.) v (stage 2;
    v, w0, w1 get no gradient), ``fit`` both stages.  The model builds lazily
    from nd + sum(field_vocab), as FM does."""

    def __init__(self, k, hidden_units, output_dim=1, activation="relu", w_reg=1e-4, v_reg=1e-4, dropout=0.2,
                 device=None, seed=None):
        super().__init__(device, seed)
        self.k = int(k)
        self.output_dim = int(output_dim)
        self.fm = FM(k, w_reg, v_reg, device=device, seed=_subseed(self._gen))
        self.dnn = DNNLayer(list(hidden_units), output_dim, activation, dropout, device=device,
                            seed=_subseed(self._gen))
        self._rest = _FnnRest(self.dnn)

    # ---- weights
    @property
    def built(self):
        return self.fm.fm.built and self.dnn._layers()[0].kernel is not None

    def build(self, n):
        """Build both models for n = nd + sum(field_vocab) one-hot columns."""
        if not self.fm.fm.built:
            self.fm.fm.build(int(n))
        if self.dnn._layers()[0].kernel is None:
            self.dnn.build(int(n) * self.k)
        self._weights_changed()

    def keras_weights(self):
        out = _prefixed("fm", self.fm.fm.keras_weights())
        out.update(_prefixed("dnn", self.dnn.keras_weights()))
        return out

    def set_keras_weights(self, weights, strict=True):
        if not self.built and "fm/v" in weights:
            self.build(torch.as_tensor(weights["fm/v"]).shape[0])
        if strict:
            unknown = set(weights) - set(self.keras_weights())
            if unknown:
                raise KeyError(f"unknown weights {sorted(unknown)}")
        _set_prefixed(self.fm.fm, "fm", weights, strict)
        _set_prefixed(self.dnn, "dnn", weights, strict)
        self._weights_changed()

    def _batch(self, dense, ids, field_offsets, field_vocab):
        """The compact batch on the device, checked: (dense [B, nd] f32, ids
        [B, F], offsets int64 [F], vocab int64 [F]); builds the model."""
        offs_h = torch.as_tensor(field_offsets, dtype=torch.int64).reshape(-1)
        voc_h = torch.as_tensor(field_vocab, dtype=torch.int64).reshape(-1)
        ids = _ids_tensor(ids, self._dev)
        if ids.dim() == 2 and ids.stride(1) != 1:
            ids = ids.contiguous()  # the kernels take a row stride only
        if ids.dim() != 2 or offs_h.numel() != ids.shape[1] or voc_h.numel() != ids.shape[1]:
            raise ValueError(f"FNN: ids {tuple(ids.shape)} need one field_offsets / field_vocab entry per column "
                             f"(got {offs_h.numel()} / {voc_h.numel()})")
        dense = _to_device_f32(dense, self._dev)
        if dense.dim() != 2 or dense.shape[0] != ids.shape[0]:
            raise ValueError(f"FNN: dense {tuple(dense.shape)} does not match ids {tuple(ids.shape)}")
        n = dense.shape[1] + int(voc_h.cpu().sum())  # (a host sum: not inside a graph capture)
        if not self.built:
            self.build(n)
        if n != self.fm.fm.v.shape[0]:
            raise ValueError(f"FNN built for {self.fm.fm.v.shape[0]} one-hot columns, got {n}")
        return dense, ids, offs_h.to(self._dev), voc_h.to(self._dev)

    def projected(self):
        """P [n, H1] = v[f] @ W1[f] (rs_fnn_project), cached on (v, W1)."""
        v, W1 = self.fm.fm.v, self.dnn._layers()[0].kernel

        def build():
            P = torch.empty(v.shape[0], W1.shape[1], dtype=torch.float32, device=self._dev)
            call("rs_fnn_project", ptr(v), ptr(W1), v.shape[0], self.k, W1.shape[1], ptr(P), _lib.stream())
            return P
        return self._packed("fnn_p", (v, W1), build)

    # ---- inference
    def fused_ok(self):
        ls = self.dnn._layers()
        if not self.built or self.output_dim != 1 or len(ls) < 2 or any(l.activation not in _lib.ACT for l in ls):
            return False
        return bool(_lib.lib().rs_fnn_ok(len(ls), ints([l.units for l in ls]),
                                         ints([_lib.ACT[l.activation] for l in ls])))

    def first_layer(self, dense, ids, field_offsets, field_vocab, check_ids=True, activate=True):
        """a1 = act(z1) (z1 with ``activate=False``) [B, H1] of the first
        Dense layer on x (.) v: rs_fnn_first_layer_fwd."""
        dense, ids, offs, voc = self._batch(dense, ids, field_offsets, field_vocab)
        first = self.dnn._layers()[0]
        B, nd = dense.shape
        out = torch.empty(B, first.units, dtype=torch.float32, device=self._dev)
        P = self.projected()
        err = _ErrFlag(self._dev)
        call("rs_fnn_first_layer_fwd", ptr(ids), _lib.id_kind(ids), ids.stride(0), ptr(dense), dense.stride(0), nd,
             ptr(offs), ptr(voc), ids.shape[1], ptr(P), P.shape[0], first.units, ptr(first.bias),
             _lib.ACT[first.activation if activate else None], ptr(out), out.stride(0), B, ptr(err.t), _lib.stream())
        if check_ids:
            err.check("FNN")
        return out

    def forward_unfused(self, dense, ids, field_offsets, field_vocab, check_ids=True):
        """The composition: rs_fnn_first_layer_fwd, then layers 2..L + the
        head as rs_mlp_fwd (layer by layer where the tower refuses them)."""
        if any(l.activation not in _lib.ACT for l in self.dnn._layers()[:1]):
            raise NotImplementedError("FNN: the first layer takes 'relu', 'sigmoid' or linear")
        a = self.first_layer(dense, ids, field_offsets, field_vocab, check_ids)
        rest = self._rest
        if rest.tower_ok():
            if self.output_dim == 1:
                return rest.tower(a, head=True)
            return sigmoid_combine(rest.tower(a))
        for layer in rest._layers():
            a = layer(a)
        return sigmoid_combine(a)

    def forward_fused(self, dense, ids, field_offsets, field_vocab, check_ids=True):
        """ids -> a1 -> tower -> sigmoid in one launch (rs_fnn_fwd)."""
        dense, ids, offs, voc = self._batch(dense, ids, field_offsets, field_vocab)
        if not self.fused_ok():
            raise ValueError("FNN.forward_fused: shape not supported (fused_ok() is False)")
        ls = self.dnn._layers()
        B, nd = dense.shape
        y = torch.empty(B, 1, dtype=torch.float32, device=self._dev)
        P = self.projected()
        err = _ErrFlag(self._dev)
        call("rs_fnn_fwd", ptr(ids), _lib.id_kind(ids), ids.stride(0), ptr(dense), dense.stride(0), nd, ptr(offs),
             ptr(voc), ids.shape[1], ptr(P), P.shape[0], ptr(ls[0].bias), len(ls), ints([l.units for l in ls]),
             ints([_lib.ACT[l.activation] for l in ls]), ptr(self._rest.prepared()), ptr(y), 1, B, ptr(err.t),
             _lib.stream())
        if check_ids:
            err.check("FNN")
        return y

    def forward_onehot(self, dense, ids, field_offsets, field_vocab, check_ids=True):
        """sigmoid(DNN(x (.) v)) [B, output_dim] on the compact batch."""
        if not self.built:
            self._batch(dense, ids, field_offsets, field_vocab)
        if self.fused_ok():
            return self.forward_fused(dense, ids, field_offsets, field_vocab, check_ids)
        return self.forward_unfused(dense, ids, field_offsets, field_vocab, check_ids)

    def forward(self, X):
        """The reference's formulation on the one-hot matrix X [B, n] (any
        dense x): (X[:, :, None] * v) reshaped to [B, n*k] through the dense
        tower (model/fnn.py:65-67).  Small n only: the input is B*n*k floats."""
        X = _to_device_f32(X, self._dev)
        B, n = X.shape
        if not self.built:
            self.build(n)
        v = self.fm.fm.v
        if n != v.shape[0]:
            raise ValueError(f"FNN built for {v.shape[0]} one-hot columns, got {n}")
        xv = (X[:, :, None] * v).reshape(B, n * self.k)
        return sigmoid_combine(self.dnn(xv))

    def fm_forward_onehot(self, dense, ids, field_offsets, field_vocab, check_ids=True):
        """The FM's own prediction (``fm_pre`` of model/fnn.py:48)."""
        return self.fm.forward_onehot(dense, ids, field_offsets, field_vocab, check_ids)

    # ---- training
    def train_step_fm(self, dense, ids, labels, field_offsets, field_vocab, lr=0.01, return_loss=False,
                      check_ids=True):
        """Stage 1: one FM.train_step (model/fnn.py:40-46).  v moves, so the
        projected table is dropped."""
        try:
            return self.fm.train_step(dense, ids, labels, field_offsets, field_vocab, lr, return_loss, check_ids)
        finally:
            self._weights_changed()

    def _check_train(self, what):
        _check_train_tower("FNN", self.dnn)
        if self.output_dim != 1:
            raise NotImplementedError(f"{what}: output_dim 1 only")

    def _stage2(self, what, dense, ids, labels, field_offsets, field_vocab, lr, want_loss, check_ids, dropout, update):
        self._check_train(what)
        dev = self._dev
        dense, ids, offs, voc = self._batch(dense, ids, field_offsets, field_vocab)
        if dev.type != "cuda":
            raise _lib.RSError(f"{what}: librs_hip kernels need device (HIP) tensors; the model is on {dev}")
        labels = _to_device_f32(labels, dev).reshape(-1)
        B, nd = dense.shape
        F = ids.shape[1]
        layers = self.dnn._layers()
        first, rest, hidden = layers[0], layers[1:], list(self.dnn.hidden_layer)
        v, W1 = self.fm.fm.v, first.kernel
        n, k, H1 = v.shape[0], self.k, first.units
        rate = _dropout_rate(self.dnn, dropout) if hidden else 0.0
        st = _lib.stream()
        emp = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
        size = _lib.lib().rs_fnn_train_workspace_size(B, nd, F, n, H1)
        if size < 0:
            _lib.check(-1, "rs_fnn_train_workspace_size")
        ws = scratch(self, "_fnn_ws", size)
        a1 = emp(B, H1)
        err = _ErrFlag(dev)
        call("rs_fnn_train_fwd", ptr(ids), _lib.id_kind(ids), ids.stride(0), ptr(dense), dense.stride(0), nd,
             ptr(offs), ptr(voc), F, ptr(v), ptr(W1), n, k, H1, ptr(first.bias), _lib.ACT[first.activation], ptr(a1),
             H1, B, ptr(ws), ptr(err.t), st)
        if check_ids:
            err.check(what)
        # Dropout after every hidden layer, the first included; the first
        # layer's multiplier is kept (the step's counter moves before dz1 is formed)
        drop = mult = None
        if rate > 0:
            rng = _dropout_rng(self)
            off0 = rng.draw(a1, rate, st)
            mult = torch.ones(B, H1, dtype=torch.float32, device=dev)
            rng.redraw(mult, rate, off0, st)
            drop = (rng, rate, [off0])
        acts = [a1]
        for layer in hidden[1:]:
            a = layer(acts[-1])
            if drop is not None:
                drop[2].append(drop[0].draw(a, rate, st))
            acts.append(a)
        logit = self.dnn.output_layer(acts[-1]) if rest else a1
        g, loss = bce_head_logit(logit.reshape(-1), labels, want_loss, st)
        if rest:
            gw = gemm_ws(self, gemm_need([(*L.kernel.shape, B) for L in rest]))
            sub = (drop[0], drop[1], drop[2][1:]) if drop is not None else None
            grads, d_a1 = _dnn_backward(rest, acts, g.view(B, 1), gw, emp, st, drop=sub)
        else:
            grads, d_a1 = [], g.view(B, 1)
        mask = a1 if first.activation == "relu" else None
        dz1 = emp(B, H1)
        g_rows = None if update else emp(min(B * (nd + F), n), H1)
        call("rs_fnn_w1_sgd", ptr(d_a1), d_a1.stride(0), ptr(mult), H1, ptr(mask), H1, ptr(dense), dense.stride(0),
             nd, F, ptr(v), ptr(W1) if update else None, n, k, H1, B, float(lr), ptr(dz1), ptr(g_rows), ptr(ws), st)
        db1 = emp(H1)
        call("rs_col_sum", ptr(dz1), H1, B, H1, ptr(db1), st)
        if update:
            _lib.sgd_update_multi(_dnn_updates(grads) + [(first.bias, db1, H1, 0.0)], lr, st)
            self._weights_changed()
            return loss
        rows = torch.cat([torch.arange(nd, device=dev).expand(B, nd), nd + offs + ids.to(torch.int64)], dim=1)
        valid = torch.cat([torch.ones(B, nd, dtype=torch.bool, device=dev),
                           (ids.to(torch.int64) >= 0) & (ids.to(torch.int64) < voc)], dim=1)
        rows = torch.unique(rows[valid])
        g_rows = g_rows[:rows.numel()]
        return {"rows": rows, "g": g_rows, "dW1": v[rows].unsqueeze(2) * g_rows.unsqueeze(1), "db1": db1,
                "layers": [(dW, db) for _, dW, db in reversed(grads)], "loss": loss}

    def train_step(self, dense, ids, labels, field_offsets, field_vocab, lr=1e-4, return_loss=False, check_ids=True,
                   dropout=None):
        """Stage 2: one step of the second fit of model/fnn.py:56-63 (SGD(lr),
        binary cross-entropy on the sigmoid output, no regulariser) on a
        compact batch.  Only the DNN trains: x (.) v is that fit's constant
        input.  rs_fnn_train_fwd sorts the B*(nd+F) lookups by row once and
        computes a1; Dropout(rate) follows every hidden layer, the first
        included (``dropout=False`` turns it off, a float overrides the
        rate); layers 2..L and the head go forward and backward as in every
        other step; rs_fnn_w1_sgd turns dL/da1 into the row-sparse rank-1
        update of W1 (a slab no sample touched is not written) and rs_col_sum
        into db1.  'relu' / linear towers, output_dim 1.  Returns the
        per-sample losses before the step if ``return_loss``."""
        return self._stage2("FNN.train_step", dense, ids, labels, field_offsets, field_vocab, lr, return_loss,
                            check_ids, dropout, True)

    def gradients(self, dense, ids, labels, field_offsets, field_vocab, check_ids=True, dropout=False):
        """What ``train_step`` would apply, without applying it: ``rows`` (the
        distinct one-hot rows of the batch, ascending), ``g`` [U, H1] (g_f per
        row), ``dW1`` [U, k, H1] (the touched slabs outer(v[f], g_f); every
        other slab's gradient is zero), ``db1``, ``layers`` [(dW, db)] of
        layers 2..L and the output Dense, and the per-sample ``loss``."""
        return self._stage2("FNN.gradients", dense, ids, labels, field_offsets, field_vocab, 0.0, True, check_ids,
                            dropout, False)

    def fit(self, dense, ids, labels, field_offsets, field_vocab, batch_size=32, epochs_fm=20, lr_fm=0.01,
            epochs_dnn=50, lr_dnn=1e-4, dropout=None):
        """The two fits of model/fnn.py:40-63 on sequential batches (no
        shuffle, as train.compile_fit): epochs_fm of the FM, then epochs_dnn
        of the DNN on x (.) v with the trained v.  Returns {'fm': [...],
        'dnn': [...]}: per epoch, the mean over the samples of the losses
        taken before each batch's step."""
        dense = _to_device_f32(dense, self._dev)
        ids = _ids_tensor(ids, self._dev)
        labels = _to_device_f32(labels, self._dev).reshape(-1)
        N, bs = ids.shape[0], int(batch_size)
        history = {"fm": [], "dnn": []}
        for name, epochs in (("fm", epochs_fm), ("dnn", epochs_dnn)):
            for _ in range(int(epochs)):
                total = torch.zeros((), dtype=torch.float64, device=self._dev)
                for b0 in range(0, N, bs):
                    sl = slice(b0, min(b0 + bs, N))
                    if name == "fm":
                        loss = self.train_step_fm(dense[sl], ids[sl], labels[sl], field_offsets, field_vocab, lr_fm,
                                                  return_loss=True)
                    else:
                        loss = self.train_step(dense[sl], ids[sl], labels[sl], field_offsets, field_vocab, lr_dnn,
                                               return_loss=True, dropout=dropout)
                    total += loss.double().sum()
                history[name].append(float(total) / max(N, 1))
        return history


_MMOE_ACTS = ("relu", "sigmoid", "linear", None)  # what rs_mmoe_fwd's towers take (tower_layer's Dense has no alpha)


class MMOE(KerasModule):
    """MMOE(mmoe_hidden_units, num_experts, num_tasks, tower_hidden_units,
    output_dim, activation='relu', use_expert_bias=True, use_gate_bias=True) —
    model/mmoe.py:10-32: a float matrix x [B, d] through mmoe_layer, then task
    t's tower_layer on task t's mix; returns num_tasks tensors [B, output_dim].
    ``train_step`` / ``fit`` train it on Keras' multi-output loss (see
    ``gradients``); the reference itself has no fit loop for MMOE.

    The mmoe_layer builds from the input width on the first call (or
    ``input_dim``); the towers are built at construction (their input is
    mmoe_hidden_units).

    ``forward_fused`` is ONE launch (rs_mmoe_fwd: experts, gates, mixes and
    tower activations stay in LDS); ``forward_unfused`` is the composition from
    the older entries (rs_dense_fwd for the experts and per gate, torch softmax
    / multiply / sum, one rs_mlp_fwd per tower).  ``forward`` takes the fused
    path when ``fused_ok()``."""

    def __init__(self, mmoe_hidden_units, num_experts, num_tasks, tower_hidden_units, output_dim, activation="relu",
                 use_expert_bias=True, use_gate_bias=True, device=None, seed=None, input_dim=None):
        super().__init__(device, seed)
        self.activation = activation
        self.output_dim = int(output_dim)
        self.mmoe_layer = mmoe_layer(mmoe_hidden_units, num_experts, num_tasks, use_expert_bias, use_gate_bias,
                                     device=device, seed=_subseed(self._gen), input_dim=input_dim)
        self.tower_layer = torch.nn.ModuleList(
            [tower_layer(tower_hidden_units, output_dim, activation, device=device, seed=_subseed(self._gen),
                         input_dim=self.mmoe_layer.hidden_units) for _ in range(self.mmoe_layer.num_tasks)])

    def build(self, d):
        self.mmoe_layer.build(d)
        self._invalidate()

    def keras_weights(self):
        out = _prefixed("mmoe_layer", self.mmoe_layer.keras_weights())
        for t, tower in enumerate(self.tower_layer):
            out.update(_prefixed(f"tower_layer_{t}", tower.keras_weights()))
        return out

    def set_keras_weights(self, weights, strict=True):
        if strict:
            unknown = set(weights) - set(self.keras_weights())
            if unknown:
                raise KeyError(f"unknown weights {sorted(unknown)}")
        _set_prefixed(self.mmoe_layer, "mmoe_layer", weights, strict)
        for t, tower in enumerate(self.tower_layer):
            _set_prefixed(tower, f"tower_layer_{t}", weights, strict)
        self._weights_changed()

    def _dims(self):
        return _mmoe_dims(self.mmoe_layer.hidden_units, list(self.tower_layer))

    def train_fused_ok(self):
        """Whether the training kernels (rs_mmoe_train_fwd / rs_mmoe_bwd) take
        this model: 'relu' or linear towers and a shape rs_mmoe_train_ok accepts."""
        m = self.mmoe_layer
        dims = self._dims()
        return bool(m.built and self.activation in ("relu", "linear", None) and len(dims) - 1 <= _MMOE_MAXL
                    and _lib.lib().rs_mmoe_train_ok(m.input_dim, m.hidden_units, m.num_experts, m.num_tasks,
                                                    len(dims) - 1, ints(dims)))

    def prepared_bwd(self):
        """The backward weight image (rs_mmoe_prepare_bwd: every tower layer's
        kernels transposed, top layer first, and W1^T), cached under the key
        of ``prepared``."""
        towers = list(self.tower_layer)

        def build():
            m = self.mmoe_layer
            dims = self._dims()
            n, ci = len(dims) - 1, ints(dims)
            img = sized("rs_mmoe_bwd_prepared_size", m.input_dim, m.hidden_units, m.num_experts, m.num_tasks, n, ci,
                        device=self._dev)
            call("rs_mmoe_prepare_bwd", m.input_dim, m.hidden_units, m.num_experts, m.num_tasks, ptr(m.expert_matrix),
                 ptrs(m.gate_matrix), n, ci, ptrs([l.kernel for tw in towers for l in tw._layers()]), ptr(img),
                 _lib.stream())
            return img
        return self._packed("mmoe_bwd", _mmoe_params(self.mmoe_layer, towers), build)

    def gradients(self, x, labels, loss_weights=None, fused=None, want_dx=False):
        """The gradients of one training step's loss without its l2 terms:
        ({Keras weight name: gradient, of the weight's shape}, the per-sample
        losses [T, B] (unweighted, before any step), dL/dx [B, d] or None).

        The loss is Keras' for a model with T outputs compiled as compile_fit
        does (utils/compile_fit.py:9-15): the per-output losses summed with
        ``loss_weights`` (default 1) — each the mean over the batch and over
        output_dim of the sigmoid cross-entropy of the tower's logits
        (BinaryCrossentropy(from_logits=True): tower_layer ends in a linear
        Dense, on which the probability form has zero gradient outside (0, 1);
        DESIGN.md "Out of scope") — plus mmoe_layer's l2(1e-4) terms, which
        ``train_step`` applies in the update.

        ``fused=True``: rs_mmoe_train_fwd (the forward's launch, which also
        stores the experts, gates, mixes and hidden activations),
        rs_mmoe_head_grad, and the whole backward data path in one launch
        (rs_mmoe_bwd: every tower delta, dz1 = [dexpert | dgate logits] and,
        with ``want_dx``, dL/dx).  ``fused=False``: rs_dense_fwd for the
        experts and per gate, torch elementwise ops for the softmax, the mix
        and their backward, _dnn_train_forward / _dnn_backward per tower.  Both
        take the weight gradients from the same deterministic blocks
        (rs_gemm(trans_a) + rs_col_sum per tensor).  ``None`` picks fused when
        ``train_fused_ok()``; ``True`` raises where the kernels refuse."""
        if self._dev.type != "cuda":
            raise NotImplementedError("MMOE.train_step: training runs only on a HIP device")
        for tw in self.tower_layer:
            _check_train_tower("MMOE", tw)
        m = self.mmoe_layer
        x = _mmoe_input(x, m)
        if fused is None:
            fused = self.train_fused_ok()
        elif fused and not self.train_fused_ok():
            raise ValueError("MMOE.train_step(fused=True): the MMOE training kernels do not take this shape")
        towers = [tw._layers() for tw in self.tower_layer]
        (B, d), H, E, T = x.shape, m.hidden_units, m.num_experts, m.num_tasks
        if B == 0:
            raise ValueError("MMOE.train_step: an empty batch")
        dims = self._dims()
        n, nout, HE, st, dev = len(dims) - 1, self.output_dim, H * E, _lib.stream(), self._dev
        emp = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
        y = mmoe_labels(labels, T, B, nout, dev)
        z = emp(T, B, nout)
        gw = gemm_ws(self, gemm_need([(d, HE, B), (d, E, B)] + [(*L.kernel.shape, B) for L in towers[0]]))
        grads = {}
        if fused:
            ci = ints(dims)
            ca = ints([_lib.ACT[self.activation]] * (n - 1) + [0])
            saved = sized("rs_mmoe_saved_size", d, H, E, T, n, ci, B, device=dev)
            call("rs_mmoe_train_fwd", ptr(x), x.stride(0), d, H, E, T, n, ci, ca, ptr(self.prepared()), ptr(saved),
                 ptr(z), z.stride(0), z.stride(1), B, st)
            G, loss = mmoe_head(z, y, loss_weights, st)
            hid = dims[1:-1]
            deltas = emp(max(B * T * sum(hid), 1))
            dz1 = emp(B, (H + T) * E)
            dx = emp(B, d) if want_dx else None
            call("rs_mmoe_bwd", ptr(saved), ptr(G), G.stride(0), d, H, E, T, n, ci, ca, ptr(self.prepared_bwd()),
                 ptr(deltas), ptr(dz1), dz1.stride(0), ptr(dx), d, B, st)
            # views of saved / deltas: layer l's input and delta, all tasks side by side
            so = B * (HE + T * E)
            ins, dels, do = [saved[so:so + B * T * H].view(B, T * H)], [], 0
            so += B * T * H
            for w in hid:
                ins.append(saved[so:so + B * T * w].view(B, T * w))
                dels.append(deltas[do:do + B * T * w].view(B, T * w))
                so, do = so + B * T * w, do + B * T * w
            dels.append(G)
            for t, layers in enumerate(towers):
                for l, L in enumerate(layers):
                    K, N = L.kernel.shape
                    dW, db, _ = dense_backward(L.kernel, ins[l][:, t * K:(t + 1) * K], dels[l][:, t * N:(t + 1) * N], gw,
                                               emp, st, d_in=False)
                    grads[(t, l)] = (dW, db)
            lg, _ = mmoe_layer_grads(m, x, dz1, gw, emp, st)
        else:
            expert = emp(B, HE)
            call("rs_dense_fwd", ptr(x), x.stride(0), ptr(m.expert_matrix), ptr(m.expert_bias), None, _lib.ACT["relu"],
                 ptr(expert), HE, B, d, HE, st)
            exp3 = expert.view(B, H, E)
            gb, ps, tacts = m.gate_bias, [], []
            for t, gm in enumerate(m.gate_matrix):
                logits = emp(B, E)
                call("rs_dense_fwd", ptr(x), x.stride(0), ptr(gm), ptr(gb[t]) if gb else None, None, 0, ptr(logits), E,
                     B, d, E, st)
                ps.append(torch.softmax(logits, dim=-1))
                mix = (exp3 * ps[t].unsqueeze(1)).sum(-1)
                acts, _ = _dnn_train_forward(self, self.tower_layer[t], mix, 0.0, st)
                self.tower_layer[t].output_layer(acts[-1], out=z[t])
                tacts.append(acts)
            G, loss = mmoe_head(z, y, loss_weights, st)
            dmix = []
            for t, layers in enumerate(towers):
                tg, below = _dnn_backward(layers, tacts[t], G[:, t * nout:(t + 1) * nout], gw, emp, st)
                for l, (_, dW, db) in enumerate(reversed(tg)):
                    grads[(t, l)] = (dW, db)
                dmix.append(below)
            dexp = torch.zeros_like(exp3)
            dlog = []
            for t in range(T):
                dexp = dexp + dmix[t].unsqueeze(2) * ps[t].unsqueeze(1)
                dp = (dmix[t].unsqueeze(2) * exp3).sum(1)
                dlog.append(ps[t] * (dp - (ps[t] * dp).sum(-1, keepdim=True)))
            dz1 = torch.cat([(dexp * (exp3 > 0)).reshape(B, HE)] + dlog, 1)
            lg, dx = mmoe_layer_grads(m, x, dz1, gw, emp, st, d_in=want_dx)
        out = {"mmoe_layer/" + k: v for k, v in lg.items()}
        for t, tw in enumerate(self.tower_layer):
            for l in range(n):
                name = f"tower_layer_{t}/" + (f"dense_{l}" if l < n - 1 else "dense_out")
                out[name + "/kernel"], out[name + "/bias"] = grads[(t, l)]
        return out, loss, dx

    def train_step(self, x, labels, lr=0.01, loss_weights=None, return_loss=False, fused=None, return_dx=False):
        """One SGD step on the multi-task loss of ``gradients`` (compile_fit's
        SGD(lr) on Keras' summed per-output losses plus the layers'
        regularisation losses): w -= lr (grad + 2 l2 w) in one
        rs_sgd_update_multi launch, l2 = 1e-4 on the mmoe_layer tensors that
        exist under the ``use_*_bias`` flags and 0 on the towers; every weight
        is updated in place.  ``labels``: a list of T arrays [B] / [B,
        output_dim] or one [T, B(, output_dim)] tensor.  Returns the
        per-sample losses [T, B] before the step if ``return_loss``, dL/dx
        [B, d] if ``return_dx``, the pair if both."""
        grads, loss, dx = self.gradients(x, labels, loss_weights, fused, return_dx)
        ups = [(p, grads[name], p.numel(), MMOE_L2 if name.startswith("mmoe_layer/") else 0.0)
               for name, p in self.keras_weights().items()]
        _lib.sgd_update_multi(ups, lr, _lib.stream())
        self._weights_changed()
        ret = tuple(v for v, want in ((loss, return_loss), (dx, return_dx)) if want)
        return None if not ret else ret[0] if len(ret) == 1 else ret

    def fit(self, x, labels, batch_size=32, epochs=10, lr=0.01, loss_weights=None):
        """compile_fit's loop (utils/compile_fit.py:14: model.fit on
        sequential batches, no shuffle) of ``train_step``.  Returns the
        history: per epoch, the mean over the samples of the tasks' losses
        summed with ``loss_weights`` (each batch's losses taken before its
        step; the l2 terms are not part of it)."""
        m = self.mmoe_layer
        x = _mmoe_input(x, m)
        B, T = x.shape[0], m.num_tasks
        y = mmoe_labels(labels, T, B, self.output_dim, self._dev)
        w = torch.ones(T, device=self._dev) if loss_weights is None else _to_device_f32(list(loss_weights), self._dev)
        history = []
        for _ in range(int(epochs)):
            total = torch.zeros((), dtype=torch.float64, device=self._dev)
            for b0 in range(0, B, int(batch_size)):
                b1 = min(b0 + int(batch_size), B)
                loss = self.train_step(x[b0:b1], y[:, b0:b1], lr, loss_weights, return_loss=True)
                total += (loss.double() * w.double().unsqueeze(1)).sum()
            history.append(float(total) / max(B, 1))
        return history

    def fused_ok(self):
        m = self.mmoe_layer
        dims = self._dims()
        return (m.built and self.activation in _MMOE_ACTS and len(dims) - 1 <= _MMOE_MAXL
                and _mmoe_ok(m.input_dim, m.hidden_units, m.num_experts, m.num_tasks, dims))

    def prepared(self):
        """The layer's and every tower's weights packed for rs_mmoe_fwd,
        cached until a weight changes."""
        towers = list(self.tower_layer)
        return self._packed("mmoe", _mmoe_params(self.mmoe_layer, towers),
                            lambda: _mmoe_prepare(self.mmoe_layer, towers, self._dev))

    def forward_fused(self, inputs, mix=None):
        """MMOE.call as ONE kernel.  mix (optional, [B, T * H]) receives the
        mmoe_layer's outputs, task t at columns t * H."""
        m = self.mmoe_layer
        x = _mmoe_input(inputs, m)
        B, d = x.shape
        dims = self._dims()
        n = len(dims) - 1
        acts = [_lib.ACT[self.activation]] * (n - 1) + [0]
        y = torch.empty(m.num_tasks, B, self.output_dim, dtype=torch.float32, device=self._dev)
        call("rs_mmoe_fwd", ptr(x), x.stride(0), d, m.hidden_units, m.num_experts, m.num_tasks, n,
             ints(dims), ints(acts), ptr(self.prepared()), ptr(mix),
             0 if mix is None else mix.stride(0), ptr(y), y.stride(0), y.stride(1), B, _lib.stream())
        return [y[t] for t in range(m.num_tasks)]

    def forward_unfused(self, inputs):
        """mmoe_layer.forward_unfused, then one DNNLayer forward per tower."""
        m = self.mmoe_layer
        mix = m.forward_unfused(_mmoe_input(inputs, m))
        H = m.hidden_units
        return [tower(mix[:, t * H:(t + 1) * H]) for t, tower in enumerate(self.tower_layer)]

    def forward(self, inputs):
        x = _mmoe_input(inputs, self.mmoe_layer)  # (builds the layer: fused_ok needs its width)
        if self.fused_ok():
            return self.forward_fused(x)
        return self.forward_unfused(x)


class DIEN(TowerMixin, KerasModule):
    """DIEN(dnn_feature_columns, history_feature_list, gru_type='GRU',
    use_negsampling=False, alpha=1.0, use_bn=False, dnn_hidden_units=(256, 128,
    64), dnn_activation='relu', att_hidden_units=(64, 16), att_activation='dice',
    att_weight_normalization=True, l2_reg_dnn=0, l2_reg_embedding=1e-6,
    dnn_dropout=0., seed=1024, task='binary') — model/dien.py:83-169.
    ``forward(inputs)`` takes the reference's feature dict (name ->
    array; ``seq_length`` holds the behaviour lengths, dien.py:197-203) and
    returns [B, 1].

    The behaviour features (``history_feature_list``, their ``hist_`` var-len
    columns) go through InterestEvolution — ONE launch from the ids when the
    shape fits (``forward``), rs_gru_fwd / composed scores / rs_augru_fwd
    otherwise and in ``forward_unfused`` — whose hist [B, D] lands in the tower
    input [every SparseFeat's row, in column order | pooled other var-len
    features | hist | dense values].  The tower DNN(dnn_hidden_units,
    dnn_activation, use_bn) + Dense(1, use_bias=False) + PredictionLayer is one
    rs_mlp_fwd launch for a BN-free 'relu' / 'sigmoid' tower (global_bias is the
    head unit's bias), composed layer by layer otherwise.  One table per
    ``embedding_name``, shared by candidate, history and negative-history
    columns.  Other var-len columns need a ``length_name`` and are pooled
    ('mean' / 'sum' / 'max') with torch ops.

    As in the reference: ``gru_type`` has no effect (AUGRU never passes it to
    its cell) and ``use_negsampling`` only adds a training loss — the ``neg_``
    columns are unused in the forward; l2 / dropout / alpha are training-only
    (``train_step``; the auxiliary loss's net is ``auxiliary_nn``, present only
    with ``use_negsampling``, with its own ``keras_weights()``).  ``augru_update='paper'`` (an extension) uses the DIEN
    paper's blend h <- (1 - z) h + z hh instead of the reference's.

    Keras weight names (``keras_weights`` / ``set_keras_weights`` round-trip;
    not verified against a live Keras graph — TensorFlow is not available to
    the tests): ``sparse_emb_{embedding_name}/embeddings`` or, when a var-len
    column shares the name, ``sparse_seq_emb_{last such column}/embeddings``;
    ``gru1/{kernel, recurrent_kernel, bias}``;
    ``attention_sequence_pooling_layer/local_att/{kernel, bias,
    dnn/kernel{i}, dnn/bias{i}, dnn/dice{i}/{dice_alpha, bn/moving_mean,
    bn/moving_variance}}``; ``gru2/{kernel, recurrent_kernel}``;
    ``dnn/{kernel{i}, bias{i}, bn{i}/{gamma, beta, moving_mean,
    moving_variance}, dice{i}/…, alpha{i}}``; ``dense/kernel``;
    ``prediction_layer/global_bias``."""

    def __init__(self, dnn_feature_columns, history_feature_list, gru_type="GRU", use_negsampling=False, alpha=1.0,
                 use_bn=False, dnn_hidden_units=(256, 128, 64), dnn_activation="relu", att_hidden_units=(64, 16),
                 att_activation="dice", att_weight_normalization=True, l2_reg_dnn=0, l2_reg_embedding=1e-6,
                 dnn_dropout=0., seed=1024, task="binary", augru_update="reference", device=None):
        super().__init__(device, seed)
        cols = list(dnn_feature_columns)
        build_input_features(cols)  # (raises the reference's TypeError on a foreign column)
        self.feature_columns, self.history_feature_list = cols, list(history_feature_list)
        self.gru_type, self.use_negsampling, self.alpha, self.task = gru_type, bool(use_negsampling), alpha, task
        self.sparse_cols = [c for c in cols if isinstance(c, SparseFeat)]
        self.dense_cols = [c for c in cols if isinstance(c, DenseFeat)]
        varlen = [c for c in cols if isinstance(c, VarLenSparseFeat)]
        hist_names = ["hist_" + n for n in self.history_feature_list]
        neg_names = ["neg_" + n for n in hist_names]
        self.history_cols = [c for c in varlen if c.name in hist_names]
        self.neg_history_cols = [c for c in varlen if c.name in neg_names]
        self.pooled_cols = [c for c in varlen if c.name not in hist_names and c.name not in neg_names]
        self.query_cols = [c for c in self.sparse_cols if c.name in self.history_feature_list]
        n_hist = len(self.history_feature_list)
        if not n_hist or len(self.history_cols) != n_hist or len(self.query_cols) != n_hist:
            raise ValueError("DIEN: every feature of history_feature_list needs a SparseFeat and a 'hist_' "
                             "VarLenSparseFeat")
        for qc, hc in zip(self.query_cols, self.history_cols):
            if hc.name != "hist_" + qc.name or hc.embedding_dim != qc.embedding_dim:
                raise ValueError(f"DIEN: behaviour columns {qc.name!r} / {hc.name!r} do not pair (order or width)")
        lens = {c.length_name for c in self.history_cols}
        if len(lens) != 1 or None in lens:
            raise ValueError("DIEN: the history columns need one common length_name")
        self.length_name = lens.pop()
        for c in self.pooled_cols:
            if c.length_name is None:
                raise ValueError(f"DIEN: var-len column {c.name!r} needs a length_name (no Keras mask reaches its "
                                 "pooling: the embeddings are built with seq_mask_zero=False)")
            if c.combiner not in ("sum", "mean", "max"):
                raise ValueError("mode must be sum or mean")
        self.maxlen = self.history_cols[0].maxlen
        # one table per embedding_name; a later var-len column replaces the entry (utils/inputs.py:33-43)
        spec = {}
        for c in self.sparse_cols:
            spec[c.embedding_name] = (f"sparse_emb_{c.embedding_name}", c)
        for c in varlen:
            spec[c.embedding_name] = (f"sparse_seq_emb_{c.name}", c)
        self._table_names = {en: kn for en, (kn, _) in spec.items()}
        self.tables = torch.nn.ParameterDict()
        for en, (kn, c) in spec.items():
            shape = (int(c.vocabulary_size), int(c.embedding_dim))
            init = c.embeddings_initializer
            w = torch.randn(*shape, generator=self._gen).mul_(1e-4) if init is None else \
                torch.as_tensor(init(shape, self._gen), dtype=torch.float32).reshape(shape)
            self.tables[en] = torch.nn.Parameter(w.to(self._dev), requires_grad=False)
        for c in cols:
            if not isinstance(c, DenseFeat) and tuple(self.tables[c.embedding_name].shape) != \
                    (int(c.vocabulary_size), int(c.embedding_dim)):
                raise ValueError(f"DIEN: column {c.name!r} does not match the table of {c.embedding_name!r}")
        D = sum(c.embedding_dim for c in self.history_cols)
        self.evolution = InterestEvolution(D, att_hidden_units, att_activation, att_weight_normalization,
                                           gru_type=gru_type, augru_update=augru_update, device=device,
                                           seed=_subseed(self._gen))
        # tower input columns
        col = 0
        self._sparse_at, self._pooled_at, self._dense_at = [], [], []
        for c in self.sparse_cols:
            self._sparse_at.append(col)
            col += c.embedding_dim
        for c in self.pooled_cols:
            self._pooled_at.append(col)
            col += c.embedding_dim
        self._hist_at = col
        col += D
        for c in self.dense_cols:
            self._dense_at.append(col)
            col += c.dimension
        self.input_width = col
        self.dnn = DNN(dnn_hidden_units, dnn_activation, l2_reg_dnn, dnn_dropout, use_bn, device=device,
                       seed=_subseed(self._gen), input_dim=col)
        self.prediction_layer = PredictionLayer(task, device=device)
        last = self.dnn.hidden_units[-1] if self.dnn.hidden_units else col
        self.dense = Dense(1, None, device=device, seed=_subseed(self._gen), input_dim=last)
        with torch.no_grad():
            self.dense.kernel.copy_(_glorot_normal(last, 1, self._gen, self._dev))
        self.dense.bias = self.prediction_layer.global_bias  # Dense(1, use_bias=False) + the head's bias: one unit
        self._l2_reg_embedding = l2_reg_embedding
        self.last_aux_loss = None
        # the auxiliary loss's net (dien.py:40), seeded after every other weight: a given seed gives the
        # same model with and without it.  Its weights are its own keras_weights(), not the model's.
        self.auxiliary_nn = DNN([100, 50, 1], "sigmoid", device=device, seed=_subseed(self._gen), input_dim=2 * D) \
            if self.use_negsampling else None

    # ---- weights
    def keras_weights(self):
        out = {f"{self._table_names[en]}/embeddings": t for en, t in self.tables.items()}
        out.update(self.evolution.keras_weights())
        out.update(_prefixed("dnn", self.dnn.keras_weights()))
        out["dense/kernel"] = self.dense.kernel
        out["prediction_layer/global_bias"] = self.prediction_layer.global_bias
        return out

    def set_keras_weights(self, weights, strict=True):
        own = self.keras_weights()
        if strict and set(own) != set(weights):
            raise KeyError(f"DIEN: missing {sorted(set(own) - set(weights))}, unknown {sorted(set(weights) - set(own))}")
        with torch.no_grad():
            for name, p in own.items():
                if name in weights:
                    p.copy_(torch.as_tensor(weights[name], dtype=torch.float32).reshape(p.shape))
        self._weights_changed()

    def _layers(self):
        return list(self.dnn.layers) + [self.dense]

    def tower_fused_ok(self):
        return (not self.dnn.use_bn and self.task in ("binary", "regression")
                and all(l.activation in ("relu", "sigmoid") for l in self.dnn.layers) and self.tower_ok())

    # ---- inputs
    def _ids(self, inputs, col, seq):
        t = _ids_tensor(inputs[col.name], self._dev)
        if seq and (t.dim() != 2 or t.shape[1] != col.maxlen):
            raise ValueError(f"DIEN: {col.name!r} has shape {tuple(t.shape)}, expected [batch, {col.maxlen}]")
        return (t if seq else t.reshape(-1)).contiguous()

    def _rows(self, ids, table, bad):
        """table[ids] with an out-of-range id as a zero row (torch ops; bad collects the flag)."""
        ok = (ids >= 0) & (ids < table.shape[0])
        bad.append(~ok.all())
        return table[torch.where(ok, ids, torch.zeros_like(ids)).long()] * ok.unsqueeze(-1)

    def _tower_input(self, inputs, err, bad):
        """[B, input_width] with every column but hist filled; the batch size."""
        first = self.sparse_cols[0] if self.sparse_cols else self.history_cols[0]
        B = int(torch.as_tensor(inputs[first.name]).shape[0])
        x = torch.empty(B, self.input_width, dtype=torch.float32, device=self._dev)
        pieces = [(c.embedding_dim, at, self._ids(inputs, c, False), self.tables[c.embedding_name])
                  for c, at in zip(self.sparse_cols, self._sparse_at)]
        for c, at in zip(self.dense_cols, self._dense_at):
            v = _to_device_f32(inputs[c.name], self._dev).reshape(B, c.dimension)
            pieces.append((c.dimension, at, v, None))
        for i in range(0, len(pieces) if B else 0, 16):
            ch = pieces[i:i + 16]
            n = len(ch)
            call("rs_concat_pieces", n, ints([p[0] for p in ch]), ints([p[1] for p in ch]),
                 ints([-1 if p[3] is None else _lib.id_kind(p[2]) for p in ch]), ptrs([p[2] for p in ch]),
                 (C.c_int64 * n)(*[p[2].stride(0) if p[3] is None else 1 for p in ch]), ptrs([p[3] for p in ch]),
                 (C.c_int64 * n)(*[0 if p[3] is None else p[3].shape[0] for p in ch]), ptr(x), x.stride(0), B,
                 ptr(err.t), _lib.stream())
        for c, at in zip(self.pooled_cols, self._pooled_at):
            ids = self._ids(inputs, c, True)
            e = self._rows(ids, self.tables[c.embedding_name], bad)
            L = torch.as_tensor(inputs[c.length_name]).reshape(-1).to(self._dev)
            m = (torch.arange(c.maxlen, device=self._dev).unsqueeze(0) < L.unsqueeze(1)).to(torch.float32).unsqueeze(-1)
            if c.combiner == "max":  # layer/sequence.py:76-78
                v = (e - (1 - m) * 1e9).max(dim=1).values
            else:
                v = (e * m).sum(1)
                if c.combiner == "mean":
                    v = v / (L.to(torch.float32).unsqueeze(1) + 1e-8)
            x[:, at:at + c.embedding_dim] = v
        return x, B

    def _tower(self, x, fused):
        if fused:
            return self.tower(x, head=self.task == "binary")
        y = self.dnn(x)
        logit = torch.empty(y.shape[0], 1, dtype=torch.float32, device=self._dev)
        if y.shape[0]:
            call("rs_dense_fwd", ptr(y), y.stride(0), ptr(self.dense.kernel), None, None, 0, ptr(logit), 1, y.shape[0],
                 y.shape[1], 1, _lib.stream())
        return self.prediction_layer(logit)

    def _check(self, err, bad, check_ids):
        if check_ids:
            err.check("DIEN")
            if bad and bool(torch.stack(bad).any()):
                raise _lib.BadIdError("DIEN: embedding id out of range (indices must be in [0, vocab))")

    def forward(self, inputs, check_ids=True):
        err, bad = _ErrFlag(self._dev), []
        x, B = self._tower_input(inputs, err, bad)
        ev, D = self.evolution, self.evolution.embedding_size
        hist_out = x[:, self._hist_at:self._hist_at + D]
        hs = [self._ids(inputs, c, True) for c in self.history_cols]
        cs = [self._ids(inputs, c, False) for c in self.query_cols]
        tabs = [self.tables[c.embedding_name] for c in self.history_cols]
        if B and ev.fused_ok(self.maxlen) and len(tabs) <= 4:
            ev.forward_ids(hs, cs, tabs, inputs[self.length_name], out=hist_out, check_ids=False, err=err)
        elif B:
            keys = torch.cat([self._rows(h, t, bad) for h, t in zip(hs, tabs)], dim=-1)
            q = torch.cat([self._rows(c, t, bad) for c, t in zip(cs, tabs)], dim=-1)
            ev(keys, q, inputs[self.length_name], out=hist_out)
        self._check(err, bad, check_ids)
        return self._tower(x, self.tower_fused_ok())

    def forward_unfused(self, inputs, check_ids=True):
        """The same forward from the stand-alone entries: torch gathers,
        rs_gru_fwd, the composed attention scores, rs_augru_fwd, then the tower
        layer by layer."""
        err, bad = _ErrFlag(self._dev), []
        x, B = self._tower_input(inputs, err, bad)
        ev, D = self.evolution, self.evolution.embedding_size
        hs = [self._ids(inputs, c, True) for c in self.history_cols]
        cs = [self._ids(inputs, c, False) for c in self.query_cols]
        tabs = [self.tables[c.embedding_name] for c in self.history_cols]
        if B:
            keys = torch.cat([self._rows(h, t, bad) for h, t in zip(hs, tabs)], dim=-1)
            q = torch.cat([self._rows(c, t, bad) for c, t in zip(cs, tabs)], dim=-1)
            ev.forward_unfused(keys, q, inputs[self.length_name], out=x[:, self._hist_at:self._hist_at + D])
        self._check(err, bad, check_ids)
        return self._tower(x, False)

    # ---- training
    def _check_train(self):
        if self._dev.type != "cuda":
            raise NotImplementedError("DIEN.train_step: training runs only on a HIP device")
        if self.task != "binary":
            raise NotImplementedError("DIEN.train_step: task 'binary' only (binary cross-entropy on the sigmoid output)")
        if any(l.activation not in ("relu", "dice") for l in self.dnn.layers):
            raise NotImplementedError("DIEN.train_step: dnn_activation 'relu' or 'dice' only")
        la = self.evolution.attention.local_att
        if la.dnn.use_bn or any(l.activation not in ("relu", "sigmoid", "dice") for l in la.dnn.layers):
            raise NotImplementedError("DIEN.train_step: att_activation 'relu', 'sigmoid' or 'dice' only")
        if any(c.combiner == "max" for c in self.pooled_cols):
            raise NotImplementedError("DIEN.train_step: pooled var-len columns train with 'sum' or 'mean' only "
                                      "('max' has no training step)")
        if self.use_negsampling:
            if len(self.neg_history_cols) != len(self.history_cols):
                raise ValueError("DIEN.train_step: use_negsampling needs a 'neg_hist_' column per behaviour feature")
            if self.maxlen < 2:
                raise ValueError("DIEN.train_step: use_negsampling needs T >= 2 (the auxiliary loss is a mean over "
                                 "B (T - 1) positions)")

    def _table_sgd(self, table, ids, grad, lr, st):
        """Row-sparse SGD of one id source of a table: ids (any shape, n
        lookups) with dL/d(row) = grad [n, k] (unit column stride);
        rs_embedding_sgd with one field at offset 0, duplicates summed in lookup
        order."""
        ids = ids.reshape(-1, 1)
        n, (V, k) = ids.shape[0], table.shape
        meta = self.__dict__.setdefault("_sgd_meta", {})
        if V not in meta:
            meta[V] = (torch.zeros(1, dtype=torch.int64, device=self._dev),
                       torch.full((1,), V, dtype=torch.int64, device=self._dev))
        ws = scratch(self, "_emb_ws", _lib.lib().rs_embedding_sgd_workspace_size(n))
        call("rs_embedding_sgd", ptr(table), V, k, ptr(ids), _lib.id_kind(ids), 1, ptr(meta[V][0]), ptr(meta[V][1]), 1,
             n, ptr(grad), grad.stride(-2), float(lr), ptr(ws), None, st)

    def train_step(self, inputs, labels, lr=0.01, return_loss=False, check_ids=True, dropout=None):
        """One step of Keras ``fit`` with SGD(lr) and binary cross-entropy on
        the sigmoid output (model/dien.py:226-231), every gradient computed
        before any update.  Returns the per-sample BCE losses [B] (before the
        step) with ``return_loss``; the scalar auxiliary loss of the step is
        left in ``last_aux_loss``.
          forward: the rows of every id source (torch gathers), then
          InterestEvolution.train_forward — rs_gru_train_fwd,
          the attention unit composed at M = B T rows (rs_din_att_concat,
          rs_dense_fwd per layer, rs_dice_train_fwd in training mode — the
          batch's statistics over all B T rows, moving averages moved with
          momentum 0.99 — or relu / sigmoid, the score Dense, mask and softmax),
          rs_augru_train_fwd, then the tower layer by layer (rs_dense_fwd,
          rs_bn_train_fwd with use_bn, relu or rs_dice_train_fwd, the dropout
          draw) and the logit;
          backward: rs_head_grad, split-K rs_gemm / rs_col_sum_split per Dense,
          rs_dice_train_bwd / rs_bn_train_bwd, then
          InterestEvolution.train_backward — rs_augru_bwd (the chain, the
          scores' gradient through the mask), the attention unit reversed into
          rs_din_att_concat_bwd, rs_gru_bwd;
          update: one rs_sgd_update_multi over the dense parameters (l2_reg_dnn
          on the tower kernels), rs_l2_decay (l2_reg_embedding) on every table
          and rs_embedding_sgd per id source (candidate, history, negative
          history, pooled 'sum' / 'mean' columns; candidates receive the
          tower-input gradient plus the attention query's).
        With ``use_negsampling`` the auxiliary loss (dien.py:20-51) is added:
        ``auxiliary_nn`` on [H1[:, :-1], keys[:, 1:]] and [H1[:, :-1],
        neg_keys[:, 1:]], mask t < len - 1, -log sigmoid as softplus, total =
        BCE + alpha aux; its weights are trained.
        relu, sigmoid and their backward (dy [y > 0], dy y (1 - y)), the masks
        and the auxiliary loss's softplus are torch elementwise ops on device
        tensors.  ``dropout``: None applies dnn_dropout, False turns it off, a
        float overrides the rate."""
        self._check_train()
        dev, st = self._dev, _lib.stream()
        ev, dnn = self.evolution, self.dnn
        D, T = ev.embedding_size, self.maxlen
        rate = 0.0 if dropout is False else float(dnn.dropout_rate or 0) if dropout in (None, True) else float(dropout)

        # ---- inputs: every id is checked before any weight changes
        err, bad = _ErrFlag(dev), []
        x, B = self._tower_input(inputs, err, bad)
        hs = [self._ids(inputs, c, True) for c in self.history_cols]
        cs = [self._ids(inputs, c, False) for c in self.query_cols]
        tabs = [self.tables[c.embedding_name] for c in self.history_cols]
        keys = torch.cat([self._rows(h, t, bad) for h, t in zip(hs, tabs)], dim=-1).contiguous()
        q = torch.cat([self._rows(c, t, bad) for c, t in zip(cs, tabs)], dim=-1).contiguous()
        ns, neg = [], None
        if self.use_negsampling:
            ns = [self._ids(inputs, c, True) for c in self.neg_history_cols]
            neg = torch.cat([self._rows(h, t, bad) for h, t in zip(ns, tabs)], dim=-1)
        self._check(err, bad, check_ids)
        labels = _to_device_f32(labels, dev).reshape(-1)
        M, M2 = B * T, B * (T - 1)
        tower = list(dnn.layers)
        aux_layers = list(self.auxiliary_nn.layers) if self.use_negsampling else []
        shapes = [(l.kernel.shape[0], l.kernel.shape[1], B) for l in tower] + [(self.dense.kernel.shape[0], 1, B)]
        shapes += [(l.kernel.shape[0], l.kernel.shape[1], 2 * M2) for l in aux_layers]
        dt = _train_ops.DenseTrain(gemm_ws(self, _train_ops.dense_train_need(shapes)), st, dev)
        updates = dt.updates  # (weight, gradient, l2)

        # ---- forward
        hist, H1, ctx = ev.train_forward(keys, q, inputs[self.length_name])
        L = ctx["L"]
        x[:, self._hist_at:self._hist_at + D] = hist
        t_in, t_pre, t_bn, t_saved = [x], [], [], []
        drop = (_dropout_rng(self), rate, []) if rate > 0 else None
        for i, l in enumerate(tower):
            z = dt.dense(t_in[-1], l, B)
            bn_saved = None
            if dnn.use_bn:
                t_bn.append(z)
                bn_saved, z = bn_train_fwd(dnn.bn_layers[i], z, st)
            saved, y = dt.act_fwd(l, z, B)
            if drop is not None:
                drop[2].append(drop[0].draw(y, rate, st))
            t_pre.append(z), t_saved.append((bn_saved, saved)), t_in.append(y)
        logit = dt.dense(t_in[-1], self.dense, B).reshape(B)
        g, loss = bce_head_logit(logit, labels, return_loss, st)

        # ---- backward: the tower
        dh = dt.dense_bwd(self.dense, t_in[-1], g.view(B, 1))
        for i in reversed(range(len(tower))):
            l = tower[i]
            if drop is not None:
                drop[0].redraw(dh, rate, drop[2][i], st)
            dz = dt.act_bwd(l, t_pre[i], t_in[i + 1], t_saved[i][1], dh, B)
            if dnn.use_bn:
                bn = dnn.bn_layers[i]
                dz, dgam, dbet = bn_train_bwd(bn, t_bn[i], t_saved[i][0], dz.contiguous(), st)
                updates.extend([(bn.gamma, dgam, 0.0), (bn.beta, dbet, 0.0)])
            dh = dt.dense_bwd(l, t_in[i], dz, l2=float(dnn.l2_reg or 0))
        if drop is not None:
            drop[0].end_step(st)
        dx = dh  # [B, input_width]

        # ---- the auxiliary loss: its gradient reaches H1[:, :-1], the history rows 1.. and the negative rows
        dh1_aux = dkeys_aux = dneg = None
        self.last_aux_loss = None
        if self.use_negsampling:
            # auxiliary_nn on the click rows then the no-click rows: one pass over 2 B (T - 1) rows
            h = H1[:, :-1].reshape(M2, D)
            u_in = [torch.cat([torch.cat([h, keys[:, 1:].reshape(M2, D)], 1),
                               torch.cat([h, neg[:, 1:].reshape(M2, D)], 1)], 0)]
            for l in aux_layers[:-1]:
                u_in.append(torch.sigmoid(dt.dense(u_in[-1], l, 2 * M2)))
            z3 = dt.dense(u_in[-1], aux_layers[-1], 2 * M2).reshape(2, B, T - 1)
            amask = (torch.arange(T - 1, device=dev).unsqueeze(0) < (L - 1).unsqueeze(1)).to(torch.float32)
            sp = torch.nn.functional.softplus
            self.last_aux_loss = ((sp(-z3[0]) + sp(z3[1])) * amask).sum() / M2
            sg = torch.sigmoid(z3)
            dz = torch.stack([(sg[0] - 1) * amask, sg[1] * amask]).mul_(float(self.alpha) / M2).reshape(2 * M2, 1)
            for i in reversed(range(len(aux_layers))):
                if i < len(aux_layers) - 1:
                    dz = dz * u_in[i + 1] * (1 - u_in[i + 1])
                dz = dt.dense_bwd(aux_layers[i], u_in[i], dz)
            zeros = lambda: torch.zeros(B, T, D, dtype=torch.float32, device=dev)
            dh1_aux, dneg = zeros(), zeros()
            dh1_aux[:, :-1] = (dz[:M2, :D] + dz[M2:, :D]).reshape(B, T - 1, D)
            dkeys_aux = dz[:M2, D:].reshape(B, T - 1, D)
            dneg[:, 1:] = dz[M2:, D:].reshape(B, T - 1, D)

        # ---- backward: the interest evolution
        dkeys, dq, ev_updates = ev.train_backward(ctx, dx[:, self._hist_at:self._hist_at + D], dh1=dh1_aux)
        updates = updates + ev_updates
        if dkeys_aux is not None:
            dkeys[:, 1:] += dkeys_aux

        # ---- update
        _lib.sgd_update_multi([(w, gr, gr.numel(), l2) for w, gr, l2 in updates], lr, st)
        l2e = float(self._l2_reg_embedding or 0)
        if l2e:
            for t in self.tables.values():
                call("rs_l2_decay", ptr(t), t.numel(), float(lr), l2e, st)
        qcol = {c.name: i for i, c in enumerate(self.query_cols)}
        offs = [0]
        for c in self.history_cols:
            offs.append(offs[-1] + c.embedding_dim)
        for c, at in zip(self.sparse_cols, self._sparse_at):
            gr = dx[:, at:at + c.embedding_dim]
            if c.name in qcol:  # a candidate: the tower-input gradient plus the attention query's
                o = offs[qcol[c.name]]
                gr = gr + dq[:, o:o + c.embedding_dim]
            self._table_sgd(self.tables[c.embedding_name], self._ids(inputs, c, False), gr.contiguous(), lr, st)
        for i, c in enumerate(self.history_cols):
            w = c.embedding_dim
            self._table_sgd(tabs[i], hs[i], dkeys[:, :, offs[i]:offs[i] + w].reshape(M, w).contiguous(), lr, st)
            if dneg is not None:
                self._table_sgd(tabs[i], ns[i], dneg[:, :, offs[i]:offs[i] + w].reshape(M, w).contiguous(), lr, st)
        for c, at in zip(self.pooled_cols, self._pooled_at):
            Lc = torch.as_tensor(inputs[c.length_name]).reshape(-1).to(dev)
            m = (torch.arange(c.maxlen, device=dev).unsqueeze(0) < Lc.unsqueeze(1)).to(torch.float32)
            if c.combiner == "mean":
                m = m / (Lc.to(torch.float32).unsqueeze(1) + 1e-8)
            gr = (m.unsqueeze(-1) * dx[:, at:at + c.embedding_dim].unsqueeze(1)).reshape(-1, c.embedding_dim)
            self._table_sgd(self.tables[c.embedding_name], self._ids(inputs, c, True), gr.contiguous(), lr, st)
        self._weights_changed()
        return loss


from .dssm import DSSM  # noqa: E402,F401  (the two-tower retrieval model: dssm.py)
