"""Keras-Layer-compatible modules for the CTR forward path, on librs_hip.so.

Each class keeps the reference layer's name, constructor arguments and
``call`` semantics (Hcyand/recommender_system, algorithm/deep_learning/layer/):

  EmbedLayer(sparse_feature_columns, k=8)     layer/core.py:267-280
  FMLayer(k, reg_w=1e-4, reg_b=1e-4)          layer/interaction.py:86-114
  CrossLayer(layer_num, reg_w, reg_b)         layer/interaction.py:49-83
  InnerProductLayer()                         layer/interaction.py:166-183
  FGCNNLayer(filters, kernel_width, dnn_maps, pooling_width)
                                              layer/interaction.py:218-258
  DNNLayer(hidden_units, output_dim, activation='relu', dropout=0.2)
                                              layer/interaction.py:30-46
  Attention(hidden_units, activation='prelu') layer/interaction.py:355-406
  Dice(axis=-1, epsilon=1e-9)                 layer/interaction.py:410-425
  ResLayer(hidden_units)                      layer/interaction.py:261-278
  WideLayer()                                 layer/interaction.py:11-26
  mmoe_layer(hidden_units, num_experts, num_tasks, use_expert_bias,
             use_gate_bias)                   layer/interaction.py:429-509
  tower_layer(hidden_units, output_dim, activation='relu')
                                              layer/interaction.py:512-523
  GRU(units, return_sequences)                Keras GRU as model/dien.py:65 uses it
  AUGRU(units, gru_type) / AUGRUCell(units)   layer/sequence.py:293-395, layer/activation.py:91-142
  LocalActivationUnit(hidden_units, activation)
                                              layer/core.py:55-108
  AttentionSequencePoolingLayer(att_hidden_units, att_activation,
      weight_normalization, return_score)     layer/sequence.py:205-273
  DNN(hidden_units, activation, use_bn, ...)  layer/core.py:123-205
  PredictionLayer(task, use_bias)             layer/core.py:223-256
  InterestEvolution(embedding_size, ...)      model/dien.py:54-80 (interest_evolution)
  SequencePoolingLayer(mode, supports_masking) layer/sequence.py:20-95
  InBatchSoftmaxLayer(sampler_config, temperature)
                                              layer/activation.py:267-285
  Dense / PReLU / BatchNormalization          the Keras layers the models use

Weights are built lazily on the first call from the input shape, like Keras
``build``, with the reference's initializers (Embedding U(-0.05,0.05),
random_normal N(0,0.05), glorot_uniform kernels, zero biases, zero PReLU/Dice
alphas, BN moving stats 0/1), and are stored in Keras orientation (Dense
kernel (in, out)).  ``keras_weights()`` / ``set_keras_weights()`` exchange them
by Keras weight name.

The forward path is inference only (Dropout is the identity, BN uses moving
statistics) and runs only on HIP device tensors through the C-ABI kernels:
there is no CPU fallback — a CPU tensor is an error.  An embedding id outside
[0, vocab) raises IndexError as TF's CPU Embedding does (the check costs one
device sync; pass ``check_ids=False`` to skip the host-side raise).
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Sequence

import torch
from torch import nn

from . import _lib
from ._lib import call, ints, ptr, ptrs, sized
from . import _train_ops
from ._train_ops import _subseed, scratch

_DEFAULT_DEVICE = "cuda"


def _device(device):
    return torch.device(device if device is not None else _DEFAULT_DEVICE)


def _stream():
    return _lib.stream()


def _to_device_f32(x, device):
    t = torch.as_tensor(x)
    if t.dtype != torch.float32:
        t = t.to(torch.float32)  # Keras Model.__call__ autocast of float inputs
    return t.to(device).contiguous()


def _ids_tensor(ids, device):
    t = torch.as_tensor(ids)
    if t.dtype == torch.float64:
        t = t.to(torch.float32)  # autocast first, then the Embedding's int cast in-kernel
    if t.dtype not in (torch.int32, torch.int64, torch.float32):
        t = t.to(torch.int64)
    return t.to(device)


class _ErrFlag:
    """Device int flag the kernels OR rs_flag bits into: an out-of-range id
    (BadIdError: an IndexError, as TF's Embedding raises) or a kernel-internal
    failure (RSError)."""

    def __init__(self, device):
        self.t = torch.zeros(1, dtype=torch.int32, device=device)

    def check(self, what):
        v = int(self.t.item())
        if v != 0:
            self.t.zero_()
            if v & ~_lib.FLAG_BAD_ID:
                raise _lib.RSError(f"{what}: kernel error flag {v:#x} ({_lib.flag_names(v)})")
            raise _lib.BadIdError(f"{what}: embedding id out of range (indices must be in [0, vocab))")


def _glorot_uniform(fan_in, fan_out, gen, device):
    lim = math.sqrt(6.0 / (fan_in + fan_out))
    return (torch.rand(fan_in, fan_out, generator=gen, device="cpu") * 2 - 1).mul_(lim).to(device)


def _normal(shape, gen, device, std=0.05):
    return torch.randn(*shape, generator=gen, device="cpu").mul_(std).to(device)


class KerasModule(nn.Module):
    """Base: Keras-named weight exchange and a seeded CPU generator for init."""

    def __init__(self, device=None, seed=None):
        super().__init__()
        self._dev = _device(device)
        self._gen = torch.Generator(device="cpu")
        self._gen.manual_seed(seed if seed is not None else torch.initial_seed() % (2 ** 31))

    def keras_weights(self) -> dict:
        return {n: p for n, p in self.named_parameters()}

    def set_keras_weights(self, weights: dict, strict: bool = True):
        own = dict(self.named_parameters())
        for name, val in weights.items():
            if name not in own:
                if strict:
                    raise KeyError(f"unknown weight {name!r}; have {sorted(own)}")
                continue
            v = torch.as_tensor(val, dtype=torch.float32).reshape(own[name].shape)
            with torch.no_grad():
                own[name].copy_(v.to(own[name].device))
        if strict:
            missing = set(own) - set(weights)
            if missing:
                raise KeyError(f"missing weights {sorted(missing)}")
        self._weights_changed()

    def _weights_changed(self):
        for m in self.modules():
            if m is not self and isinstance(m, KerasModule):
                m._invalidate()
        self._invalidate()

    def _packed(self, slot, params, build, extra=()):
        """The one cache of everything packed from weights (MFMA operand
        images, backward images, folded affines): ``build()``'s value for
        `slot`, rebuilt when a parameter's version or storage, or `extra`,
        differs from the last build.  One entry per slot; the entry holds the
        value, so whatever ``build`` returns beside the image (operands a
        stream still reads) lives as long as the image does.  The training
        steps move weights through raw pointers, which bumps no version: they
        end in ``_weights_changed()``.  The dict lives in ``__dict__`` only —
        not a Module attribute, not in ``state_dict``."""
        key = (extra, tuple((p._version, p.data_ptr()) for p in params))
        cache = self.__dict__.setdefault("_packed_cache", {})
        ent = cache.get(slot)
        if ent is None or ent[0] != key:
            ent = cache[slot] = (key, build())
        return ent[1]

    def _invalidate(self):
        self.__dict__.pop("_packed_cache", None)


# --------------------------------------------------------------- embedding
class EmbedLayer(KerasModule):
    """EmbedLayer(sparse_feature_columns, k=8) — layer/core.py:267-280.

    One Keras ``Embedding(feat_onehot_dim, k)`` per sparse field, stored as ONE
    contiguous [sum(vocab), k] HBM table (64-B rows at k=16) with per-field row
    offsets; ``field_table(i)`` is field i's Embedding matrix (a view).
    ``forward(sparse)`` returns the flattened [B, F*k] (field-major), exactly
    like the reference (which ignores feat['embed_dim'] and uses k).
    """

    def host_meta(self):
        """(offsets, vocab) as host int64 arrays (addresses), for the entry
        points that take the field metadata by value."""
        return C.addressof(self._host_offsets), C.addressof(self._host_vocab)

    def __init__(self, sparse_feature_columns, k=8, device=None, seed=None):
        super().__init__(device, seed)
        self.k = int(k)
        self.vocab_sizes = [int(f["feat_onehot_dim"]) for f in sparse_feature_columns]
        self.n_fields = len(self.vocab_sizes)
        offs = [0]
        for v in self.vocab_sizes[:-1]:
            offs.append(offs[-1] + v)
        self.row_offsets = offs
        self.total_rows = sum(self.vocab_sizes)
        self.register_buffer("field_offsets", torch.tensor(offs, dtype=torch.int64, device=self._dev))
        self.register_buffer("field_vocab", torch.tensor(self.vocab_sizes, dtype=torch.int64, device=self._dev))
        # host copies of the same metadata (rs_embed_fm_fwd_hm: kernel arguments)
        F = max(self.n_fields, 1)
        self._host_offsets = (C.c_int64 * F)(*offs[:self.n_fields])
        self._host_vocab = (C.c_int64 * F)(*self.vocab_sizes)
        table = torch.empty(self.total_rows, self.k, dtype=torch.float32, device=self._dev)
        if table.is_cuda:
            g = torch.Generator(device=table.device)
            g.manual_seed(int(torch.randint(0, 2 ** 31, (1,), generator=self._gen)))
            table.uniform_(-0.05, 0.05, generator=g)
        else:
            table.uniform_(-0.05, 0.05, generator=self._gen)
        self.table = nn.Parameter(table, requires_grad=False)
        self._err = _ErrFlag(self._dev)

    def field_table(self, i: int) -> torch.Tensor:
        o = self.row_offsets[i]
        return self.table[o:o + self.vocab_sizes[i]]

    def keras_weights(self):
        return {f"embedding_{i}/embeddings": self.field_table(i) for i in range(self.n_fields)}

    def set_keras_weights(self, weights, strict=True):
        for i in range(self.n_fields):
            name = f"embedding_{i}/embeddings"
            if name in weights:
                with torch.no_grad():
                    self.field_table(i).copy_(torch.as_tensor(weights[name], dtype=torch.float32).to(self._dev))
            elif strict:
                raise KeyError(f"missing weight {name}")

    def gather(self, ids, dense=None, out=None, check_ids=True):
        """x = [dense | emb] in one launch (rs_embed_gather)."""
        ids = _ids_tensor(ids, self._dev)
        B = ids.shape[0]
        nd = 0 if dense is None else dense.shape[1]
        d = nd + self.n_fields * self.k
        if out is None:
            out = torch.empty(B, d, dtype=torch.float32, device=self._dev)
        call("rs_embed_gather", ptr(ids), _lib.id_kind(ids), ids.stride(0), ptr(dense),
             0 if dense is None else dense.stride(0), nd, ptr(self.table), ptr(self.field_offsets),
             ptr(self.field_vocab), self.n_fields, self.k, ptr(out), out.stride(0), B, ptr(self._err.t), _stream())
        if check_ids:
            self._err.check("EmbedLayer")
        return out

    def forward(self, inputs, check_ids=True):
        if inputs.shape[1] != self.n_fields:
            raise ValueError(f"EmbedLayer expects {self.n_fields} sparse columns, got {inputs.shape[1]}")
        return self.gather(inputs, check_ids=check_ids)


# ---------------------------------------------------------------------- FM
class FMLayer(KerasModule):
    """FMLayer(k, reg_w=1e-4, reg_b=1e-4) — layer/interaction.py:86-114.

    Weights w0:(1,) zeros, w1:(n,1) and v:(n,k) ~ N(0, 0.05), built from the
    input width on the first call.  The regularisers only affect training
    losses and are kept as attributes.  ``forward(x[B,n]) -> [B,1]``.
    """

    def __init__(self, k, reg_w=1e-4, reg_b=1e-4, device=None, seed=None, input_dim=None):
        super().__init__(device, seed)
        self.k = int(k)
        self.reg_w, self.reg_b = reg_w, reg_b
        self.w0 = self.w1 = self.v = None
        if input_dim is not None:
            self.build(input_dim)

    def build(self, n):
        self.w0 = nn.Parameter(torch.zeros(1, device=self._dev), requires_grad=False)
        self.w1 = nn.Parameter(_normal((n, 1), self._gen, self._dev), requires_grad=False)
        self.v = nn.Parameter(_normal((n, self.k), self._gen, self._dev), requires_grad=False)
        self._invalidate()

    @property
    def built(self):
        return self.v is not None

    def prepared(self, nd, n_fields, emb_k):
        """Packed MFMA operand image of (w1, v) for a given x layout (one
        image: another layout repacks)."""
        def build():
            n = _lib.lib().rs_fm_prepared_size(nd, n_fields, emb_k, self.k)
            if n <= 0:
                raise ValueError("FMLayer: unsupported shape")
            prep = torch.empty(n, dtype=torch.float32, device=self._dev)
            call("rs_fm_prepare", ptr(self.w1), ptr(self.v), nd, n_fields, emb_k, self.k, ptr(prep), _stream())
            return prep
        return self._packed("fm", (self.w1, self.v), build, extra=(nd, n_fields, emb_k))

    def forward(self, inputs):
        x = _to_device_f32(inputs, self._dev)
        if not self.built:
            self.build(x.shape[-1])
        B, n = x.shape
        if n != self.w1.shape[0]:
            raise ValueError(f"FMLayer built for {self.w1.shape[0]} inputs, got {n}")
        out = torch.empty(B, 1, dtype=torch.float32, device=self._dev)
        prep = self.prepared(n, 0, 0)
        call("rs_fm_fwd", ptr(x), x.stride(0), n, ptr(prep), ptr(self.w0), self.k, ptr(out), B, _stream())
        return out


# --------------------------------------------------------------- DCN cross
class CrossLayer(KerasModule):
    """CrossLayer(layer_num, reg_w=1e-4, reg_b=1e-4) — layer/interaction.py:49-83.
    Weights w{i}, b{i}: (d,1) ~ N(0, 0.05).  ``forward(x[B,d]) -> [B,d]``."""

    def __init__(self, layer_num, reg_w=1e-4, reg_b=1e-4, device=None, seed=None, input_dim=None):
        super().__init__(device, seed)
        self.layer_num = int(layer_num)
        self.reg_w, self.reg_b = reg_w, reg_b
        self.cross_weight = nn.ParameterList()
        self.cross_bias = nn.ParameterList()
        if input_dim is not None:
            self.build(input_dim)

    def build(self, d):
        for _ in range(self.layer_num):
            self.cross_weight.append(nn.Parameter(_normal((d, 1), self._gen, self._dev), requires_grad=False))
        for _ in range(self.layer_num):
            self.cross_bias.append(nn.Parameter(_normal((d, 1), self._gen, self._dev), requires_grad=False))
        self._invalidate()

    @property
    def built(self):
        return len(self.cross_weight) == self.layer_num and (self.layer_num == 0 or len(self.cross_bias) > 0)

    def keras_weights(self):
        out = {f"w{i}": w for i, w in enumerate(self.cross_weight)}
        out.update({f"b{i}": b for i, b in enumerate(self.cross_bias)})
        return out

    def set_keras_weights(self, weights, strict=True):
        for i in range(self.layer_num):
            with torch.no_grad():
                self.cross_weight[i].copy_(torch.as_tensor(weights[f"w{i}"], dtype=torch.float32).reshape(-1, 1))
                self.cross_bias[i].copy_(torch.as_tensor(weights[f"b{i}"], dtype=torch.float32).reshape(-1, 1))
        self._invalidate()

    def prepared(self, d):
        def build():
            L = self.layer_num
            prep = sized("rs_cross_prepared_size", d, L, device=self._dev)
            if L:
                W = torch.stack([w.reshape(-1) for w in self.cross_weight]).contiguous()
                Bb = torch.stack([b.reshape(-1) for b in self.cross_bias]).contiguous()
            else:
                W = Bb = None
            call("rs_cross_prepare", ptr(W), ptr(Bb), d, L, ptr(prep), _stream())
            return prep, (W, Bb)  # the stacked operands: stream-ordered lifetime
        return self._packed("cross", list(self.cross_weight) + list(self.cross_bias), build)[0]

    def forward(self, inputs, out=None):
        x = _to_device_f32(inputs, self._dev)
        if not self.built:
            self.build(x.shape[1])
        B, d = x.shape
        if out is None:
            out = torch.empty(B, d, dtype=torch.float32, device=self._dev)
        call("rs_cross_fwd", ptr(x), x.stride(0), d, self.layer_num, ptr(self.prepared(d)), ptr(out), out.stride(0),
             B, _stream())
        return out


# ------------------------------------------------------ PNN inner product
class InnerProductLayer(KerasModule):
    """InnerProductLayer() — layer/interaction.py:166-183.
    ``forward(e[B,F,k]) -> [B, F(F-1)/2]``, pairs (i<j) row-major."""

    def __init__(self, device=None):
        super().__init__(device)

    def forward(self, inputs, out=None):
        e = _to_device_f32(inputs, self._dev)
        B, F, k = e.shape
        P = F * (F - 1) // 2
        if out is None:
            out = torch.empty(B, P, dtype=torch.float32, device=self._dev)
        call("rs_inner_product_fwd", ptr(e), F, k, ptr(out), out.stride(0), B, _stream())
        return out


class OuterProductLayer(KerasModule):
    """OuterProductLayer() — layer/interaction.py:186-215.  Weight W:
    (k, P, k) ~ N(0, 0.05) (tf.random_normal_initializer()), built on the
    first call.  ``forward(e[B,F,k]) -> [B,P]`` with
    out[b,p] = sum_{a,j} e[b,row_p,j] W[a,p,j] e[b,col_p,a]."""

    def __init__(self, device=None, seed=None):
        super().__init__(device, seed)
        self.W = None
        self.field_num = self.k = None

    def build(self, F, k):
        self.field_num, self.k = int(F), int(k)
        P = F * (F - 1) // 2
        self.W = nn.Parameter(_normal((k, P, k), self._gen, self._dev), requires_grad=False)

    def keras_weights(self):
        return {"W": self.W}

    def set_keras_weights(self, weights, strict=True):
        with torch.no_grad():
            self.W.copy_(torch.as_tensor(weights["W"], dtype=torch.float32).reshape(self.W.shape))

    def prepared(self):
        """W packed into per-lane MFMA fragments (rs_outer_prepare), cached."""
        def build():
            prep = sized("rs_outer_prepared_size", self.field_num, self.k, device=self._dev)
            call("rs_outer_prepare", ptr(self.W), self.field_num, self.k, ptr(prep), _stream())
            return prep
        return self._packed("outer", (self.W,), build)

    def forward(self, inputs, out=None):
        e = _to_device_f32(inputs, self._dev)
        B, F, k = e.shape
        if self.W is None:
            self.build(F, k)
        if (F, k) != (self.field_num, self.k):
            raise ValueError(f"OuterProductLayer built for F={self.field_num}, k={self.k}; got {F}, {k}")
        P = F * (F - 1) // 2
        if out is None:
            out = torch.empty(B, P, dtype=torch.float32, device=self._dev)
        call("rs_outer_product_fwd", ptr(e.contiguous()), F, k, ptr(self.prepared()), ptr(out), out.stride(0), B,
             _stream())
        return out


class FGCNNLayer(KerasModule):
    """FGCNNLayer(filters=[14,16], kernel_width=[7,7], dnn_maps=[3,3],
    pooling_width=[2,2]) — layer/interaction.py:218-258.  Per layer
    Conv2D(filters, (kernel_width, 1), 'same', tanh) along the field axis,
    MaxPool2D((pooling_width, 1)), Flatten, Dense(dnn_maps * H' * k, relu),
    reshaped to [B, dnn_maps * H', k]; the layers' results are concatenated
    along the field axis.  ``forward(e[B,F,k]) -> [B, n_new, k]``.

    The whole conv stack is ONE launch (rs_fgcnn_conv_fwd, or
    rs_embed_fgcnn_conv_fwd straight from ids); each recombination Dense is
    rs_dense_fwd on the launch's workspace.  Deviation: the reference builds
    the recombination Dense layers inside ``call`` (fresh weights per call);
    here they are built once (glorot-uniform kernel, zero bias) and exchanged
    by name: conv_i/kernel [kw, 1, Cin, Cout], conv_i/bias, dense_i/kernel,
    dense_i/bias."""

    def __init__(self, filters=(14, 16), kernel_width=(7, 7), dnn_maps=(3, 3), pooling_width=(2, 2), device=None,
                 seed=None):
        super().__init__(device, seed)
        self.filters = [int(v) for v in filters]
        self.kernel_width = [int(v) for v in kernel_width]
        self.dnn_maps = [int(v) for v in dnn_maps]
        self.pooling_width = [int(v) for v in pooling_width]
        n = len(self.filters)
        if not (len(self.kernel_width) == len(self.dnn_maps) == len(self.pooling_width) == n):
            raise ValueError("FGCNNLayer: filters, kernel_width, dnn_maps and pooling_width need one entry per layer")
        if any(m < 1 for m in self.dnn_maps):
            raise ValueError("FGCNNLayer: dnn_maps must be >= 1")
        self.conv_kernels = nn.ParameterList()
        self.conv_biases = nn.ParameterList()
        self.dense_layers = nn.ModuleList()
        self.field_num = self.k = None

    @property
    def built(self):
        return self.field_num is not None

    def _cfg(self):
        return len(self.filters), ints(self.filters), ints(self.kernel_width), ints(self.pooling_width)

    def build(self, F, k):
        F, k = int(F), int(k)
        ws = _lib.lib().rs_fgcnn_workspace_size(F, k, *self._cfg())
        if ws < 0:
            _lib.check(-1, "rs_fgcnn_workspace_size")
        self.ws_size = int(ws)
        self.pooled_shapes, self.new_fields = [], []  # per layer (H', k, Cout) and dnn_maps * H'
        H, cin = F, 1
        for cout, kw, maps, pw in zip(self.filters, self.kernel_width, self.dnn_maps, self.pooling_width):
            # Keras Conv2D glorot_uniform: fans = receptive field (kw * 1) x channels
            lim = math.sqrt(6.0 / (kw * cin + kw * cout))
            w = (torch.rand(kw, 1, cin, cout, generator=self._gen, device="cpu") * 2 - 1).mul_(lim)
            self.conv_kernels.append(nn.Parameter(w.to(self._dev), requires_grad=False))
            self.conv_biases.append(nn.Parameter(torch.zeros(cout, device=self._dev), requires_grad=False))
            H = H // pw
            self.pooled_shapes.append((H, k, cout))
            self.new_fields.append(maps * H)
            self.dense_layers.append(Dense(maps * H * k, "relu", device=self._dev, seed=_subseed(self._gen),
                                           input_dim=H * k * cout))
            cin = cout
        self.n_new = sum(self.new_fields)
        self.field_num, self.k = F, k

    def keras_weights(self):
        out = {}
        for i, (w, b, d) in enumerate(zip(self.conv_kernels, self.conv_biases, self.dense_layers)):
            out[f"conv_{i}/kernel"], out[f"conv_{i}/bias"] = w, b
            out[f"dense_{i}/kernel"], out[f"dense_{i}/bias"] = d.kernel, d.bias
        return out

    def set_keras_weights(self, weights, strict=True):
        own = self.keras_weights()
        if strict and set(own) != set(weights):
            raise KeyError(f"FGCNNLayer: expected weights {sorted(own)}, got {sorted(weights)}")
        with torch.no_grad():
            for name, p in own.items():
                if name in weights:
                    p.copy_(torch.as_tensor(weights[name], dtype=torch.float32).reshape(p.shape))

    def _weight_ptrs(self):
        return ptrs(self.conv_kernels), ptrs(self.conv_biases)

    def _check_shape(self, F, k):
        if not self.built:
            self.build(F, k)
        if (F, k) != (self.field_num, self.k):
            raise ValueError(f"FGCNNLayer built for F={self.field_num}, k={self.k}; got {F}, {k}")

    def conv(self, e, ws=None):
        """The conv stack on e [B,F,k]: every layer's pooled map, flattened in
        Keras order, side by side in ws [B, ws_size] (one launch)."""
        e = _to_device_f32(e, self._dev)
        B, F, k = e.shape
        self._check_shape(F, k)
        if ws is None:
            ws = torch.empty(B, self.ws_size, dtype=torch.float32, device=self._dev)
        cw, cb = self._weight_ptrs()
        call("rs_fgcnn_conv_fwd", ptr(e), F, k, *self._cfg(), cw, cb, ptr(ws), ws.stride(0), B, _stream())
        return ws

    def conv_ids(self, ids, embed, z, err, ws=None):
        """The conv stack straight from ids [B,F] through EmbedLayer `embed`;
        the gathered rows also land in z[:, :F*k] (one launch)."""
        B = ids.shape[0]
        self._check_shape(embed.n_fields, embed.k)
        if ws is None:
            ws = torch.empty(B, self.ws_size, dtype=torch.float32, device=self._dev)
        cw, cb = self._weight_ptrs()
        call("rs_embed_fgcnn_conv_fwd", ptr(ids), _lib.id_kind(ids), ids.stride(0), ptr(embed.table),
             ptr(embed.field_offsets), ptr(embed.field_vocab), embed.n_fields, embed.k, *self._cfg(), cw, cb, ptr(ws),
             ws.stride(0), ptr(z), 0 if z is None else z.stride(0), B, ptr(err), _stream())
        return ws

    def recombine(self, ws, out, col=0):
        """Dense(dnn_maps * H' * k, relu) of every layer's pooled map, written
        side by side into out[:, col:col + n_new*k] (one rs_dense_fwd each)."""
        off = 0
        for (H, k, cout), d in zip(self.pooled_shapes, self.dense_layers):
            n = H * k * cout
            d(ws[:, off:off + n], out=out[:, col:col + d.units])
            off += n
            col += d.units
        return out

    def forward(self, inputs):
        e = _to_device_f32(inputs, self._dev)
        ws = self.conv(e)
        out = torch.empty(e.shape[0], self.n_new * self.k, dtype=torch.float32, device=self._dev)
        return self.recombine(ws, out).view(e.shape[0], self.n_new, self.k)

    def bwd_workspace_size(self, B):
        """Bytes of rs_fgcnn_conv_bwd's workspace at batch B; raises RSError
        where the backward's per-sample tile does not fit in LDS."""
        n = _lib.lib().rs_fgcnn_conv_bwd_workspace_size(self.field_num, self.k, *self._cfg(), int(B))
        if n < 0:
            _lib.check(-1, "rs_fgcnn_conv_bwd_workspace_size")
        return int(n)

    def backward(self, rows, ws, new, dnew, de):
        """The layer's backward from dnew = dL/d(output) [B, n_new*k].  ``rows``
        [B, >= F*k] holds the input rows in its first F*k columns, ``ws`` is the
        forward's workspace and ``new`` its output (after the relu); all three
        may be column views.  Per layer the recombination Dense: dpre = dnew
        [new > 0], dkernel = ws_i^T dpre (rs_gemm), dbias (rs_col_sum), dws_i =
        dpre kernel^T (rs_gemm into its columns of dws); then ONE
        rs_fgcnn_conv_bwd launch ADDS dL/d(rows) into de [B, F*k] and writes
        the conv kernels' and biases' gradients.  Returns {name: gradient},
        keyed like keras_weights()."""
        B, st = rows.shape[0], _stream()
        emp = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=self._dev)
        grads = {}
        dws = emp(B, self.ws_size)
        shapes = [(*d.kernel.shape, B) for d in self.dense_layers] + [(B, *d.kernel.shape) for d in self.dense_layers]
        gw = _train_ops.gemm_ws(self, _train_ops.gemm_need(shapes))
        off = col = 0
        for i, ((H, k, cout), d) in enumerate(zip(self.pooled_shapes, self.dense_layers)):
            n, u = H * k * cout, d.units
            dpre = dnew[:, col:col + u] * (new[:, col:col + u] > 0)
            dW, db, _ = _train_ops.dense_backward(d.kernel, ws[:, off:off + n], dpre, gw, emp, st, d_in=False)
            grads[f"dense_{i}/kernel"], grads[f"dense_{i}/bias"] = dW, db
            call("rs_gemm", 0, 1, B, n, u, 1.0, ptr(dpre), u, ptr(d.kernel), u, 0.0, dws.data_ptr() + 4 * off,
                 self.ws_size, None, 0, *gw, st)
            off += n
            col += u
        dcw = [emp(*w.shape) for w in self.conv_kernels]
        dcb = [emp(*b.shape) for b in self.conv_biases]
        cws = scratch(self, "_bwd_ws", max(self.bwd_workspace_size(B), 1))
        call("rs_fgcnn_conv_bwd", ptr(rows), rows.stride(0), ptr(ws), ws.stride(0), ptr(dws), dws.stride(0),
             self.field_num, self.k, *self._cfg(), ptrs(self.conv_kernels), ptr(de), de.stride(0), ptrs(dcw), ptrs(dcb),
             ptr(cws), cws.numel(), B, st)
        for i in range(len(dcw)):
            grads[f"conv_{i}/kernel"], grads[f"conv_{i}/bias"] = dcw[i], dcb[i]
        return grads


# -------------------------------------------------------------- dense / MLP
_MLP_MAXL, _MLP_MAXD = 8, 1024  # rs_mlp_fwd limits (mlp.hip)
_ACTS = ("relu", "prelu", "sigmoid", "linear", None, "dice")


class Dense(KerasModule):
    """Keras Dense(units, activation) on 2-D inputs: kernel (in, units)
    glorot-uniform, bias zeros.  activation: None/'linear', 'relu', 'sigmoid',
    'prelu' (Keras PReLU(): alpha shape [units], zeros) or 'dice' (Dice())."""

    def __init__(self, units, activation=None, device=None, seed=None, input_dim=None):
        super().__init__(device, seed)
        if activation not in _ACTS:
            raise ValueError(f"unsupported activation {activation!r}")
        self.units = int(units)
        self.activation = activation
        self.kernel = self.bias = self.alpha = None
        self.dice = None
        if input_dim is not None:
            self.build(input_dim)

    def build(self, n):
        self.kernel = nn.Parameter(_glorot_uniform(n, self.units, self._gen, self._dev), requires_grad=False)
        self.bias = nn.Parameter(torch.zeros(self.units, device=self._dev), requires_grad=False)
        if self.activation == "prelu":
            self.alpha = nn.Parameter(torch.zeros(self.units, device=self._dev), requires_grad=False)
        if self.activation == "dice":
            self.dice = Dice(device=self._dev)
            self.dice.build(self.units)

    def keras_weights(self):
        out = {"kernel": self.kernel, "bias": self.bias}
        if self.alpha is not None:
            out["alpha"] = self.alpha
        if self.dice is not None:
            out.update({f"dice/{k}": v for k, v in self.dice.keras_weights().items()})
        return out

    def set_keras_weights(self, weights, strict=True):
        with torch.no_grad():
            self.kernel.copy_(torch.as_tensor(weights["kernel"], dtype=torch.float32))
            self.bias.copy_(torch.as_tensor(weights["bias"], dtype=torch.float32))
            if self.alpha is not None:
                self.alpha.copy_(torch.as_tensor(weights["alpha"], dtype=torch.float32).reshape(-1))
        if self.dice is not None:
            self.dice.set_keras_weights({k[5:]: v for k, v in weights.items() if k.startswith("dice/")}, strict)

    def forward(self, inputs, out=None):
        x = _to_device_f32(inputs, self._dev) if not (torch.is_tensor(inputs) and inputs.is_cuda) else inputs
        if self.kernel is None:
            self.build(x.shape[-1])
        M, K = x.shape
        if out is None:
            out = torch.empty(M, self.units, dtype=torch.float32, device=self._dev)
        act = 0 if self.activation == "dice" else _lib.ACT[self.activation]
        call("rs_dense_fwd", ptr(x), x.stride(0), ptr(self.kernel), ptr(self.bias), ptr(self.alpha), act, ptr(out),
             out.stride(0), M, K, self.units, _stream())
        if self.activation == "dice":
            out = self.dice(out, out=out)
        return out


class TowerMixin:
    """A stack of Keras Dense layers run as ONE rs_mlp_fwd launch (mlp.hip):
    activations stay in LDS, weights are packed once.  The host class
    provides ``_layers()`` (the Dense layers in order) and ``_dev``."""

    def tower_ok(self):
        ls = self._layers()
        if not (ls[0].kernel is not None and len(ls) <= _MLP_MAXL and all(l.activation != "dice" for l in ls)
                and all(d <= _MLP_MAXD for d in self._dims())):
            return False
        dims = self._dims()
        return _lib.lib().rs_mlp_prepared_size(len(ls), ints(dims)) >= 0  # LDS budget

    def _dims(self):
        ls = self._layers()
        return [ls[0].kernel.shape[0]] + [l.units for l in ls]

    def prepared(self, in_rows=None):
        """Weights packed in MFMA B-fragment order (rs_mlp_prepare), cached
        until any weight changes (in-place updates bump tensor versions)."""
        ls = self._layers()
        params = [p for l in ls for p in (l.kernel, l.bias, l.alpha) if p is not None]

        def build():
            n, ci = len(ls), ints(self._dims())
            prep = sized("rs_mlp_prepared_size", n, ci, device=self._dev)
            call("rs_mlp_prepare", n, ci, ptrs([l.kernel for l in ls]), ptrs([l.bias for l in ls]),
                 ptrs([l.alpha for l in ls]), ptr(in_rows), ptr(prep), _stream())
            return prep, in_rows  # in_rows kept alive with its packing
        slot, extra = (None, ()) if in_rows is None else (in_rows.data_ptr(), (in_rows._version,))
        return self._packed(("tower", slot), params, build, extra)[0]

    def tower(self, x, extra=None, c0=1.0, c1=1.0, head=False, out=None, in_affine=None):
        """rs_mlp_fwd on x:[M, K] (device, row stride x.stride(0)).  head=True:
        sigmoid(c0*dnn + c1*extra) (output_dim 1).  in_affine=(scale, shift):
        the tower runs on x * scale + shift (an inference BatchNormalization
        folded into the launch: rs_mlp_affine_fwd)."""
        ls = self._layers()
        n = len(ls)
        dims = self._dims()
        M = x.shape[0]
        if out is None:
            out = torch.empty(M, 1 if head else dims[-1], dtype=torch.float32, device=self._dev)
        acts = [_lib.ACT[l.activation] for l in ls]
        if in_affine is not None:
            sc, sh = in_affine
            if sc.numel() != dims[0] or sh.numel() != dims[0]:
                raise ValueError(f"tower: in_affine needs {dims[0]} scales and shifts")
            call("rs_mlp_affine_fwd", ptr(x), x.stride(0), ptr(sc), ptr(sh), n, ints(dims),
                 ints(acts), ptr(self.prepared()), ptr(out), out.stride(0), 1 if head else 0, ptr(extra),
                 float(c0), float(c1), M, _stream())
            return out
        call("rs_mlp_fwd", ptr(x), x.stride(0), n, ints(dims), ints(acts),
             ptr(self.prepared()), ptr(out), out.stride(0), 1 if head else 0, ptr(extra), float(c0), float(c1), M,
             _stream())
        return out


class DNNLayer(TowerMixin, KerasModule):
    """DNNLayer(hidden_units, output_dim, activation='relu', dropout=0.2) —
    layer/interaction.py:30-46.  Dropout is inactive at inference."""

    def __init__(self, hidden_units, output_dim, activation="relu", dropout=0.2, device=None, seed=None):
        super().__init__(device, seed)
        self.dropout = dropout
        self.hidden_layer = nn.ModuleList(
            [Dense(u, activation=activation, device=device, seed=int(torch.randint(0, 2 ** 31, (1,), generator=self._gen)))
             for u in hidden_units])
        self.output_layer = Dense(output_dim, activation=None, device=device,
                                  seed=int(torch.randint(0, 2 ** 31, (1,), generator=self._gen)))

    def _layers(self):
        return list(self.hidden_layer) + [self.output_layer]

    def keras_weights(self):
        out = {}
        for i, l in enumerate(self.hidden_layer):
            out.update({f"dense_{i}/{k}": v for k, v in l.keras_weights().items()})
        out.update({f"dense_out/{k}": v for k, v in self.output_layer.keras_weights().items()})
        return out

    def set_keras_weights(self, weights, strict=True):
        for i, l in enumerate(self.hidden_layer):
            l.set_keras_weights({k.split("/", 1)[1]: v for k, v in weights.items() if k.startswith(f"dense_{i}/")},
                                strict)
        self.output_layer.set_keras_weights(
            {k.split("/", 1)[1]: v for k, v in weights.items() if k.startswith("dense_out/")}, strict)

    def build(self, n):
        for layer in self.hidden_layer:
            layer.build(n)
            n = layer.units
        self.output_layer.build(n)

    def forward(self, inputs):
        x = inputs
        if torch.is_tensor(x) and x.is_cuda and x.dim() == 2 and x.stride(1) == 1 and self.output_layer.kernel is not None \
                and self.tower_ok():
            return self.tower(x)
        for layer in self.hidden_layer:
            x = layer(x)
        return self.output_layer(x)


class Dice(KerasModule):
    """Dice(axis=-1, epsilon=1e-9) at inference — layer/interaction.py:410-425:
    BN(center=False, scale=False) with moving stats, p = sigmoid(xhat),
    y = alpha*(1-p)*x + p*x.  alpha, moving_mean: zeros; moving_variance: ones."""

    def __init__(self, axis=-1, epsilon=1e-9, device=None):
        super().__init__(device)
        if axis != -1:
            raise NotImplementedError("Dice: only axis=-1 (the reference default) is supported")
        self.axis, self.epsilon = axis, float(epsilon)
        self.alphas = self.moving_mean = self.moving_variance = None

    def build(self, n):
        self.alphas = nn.Parameter(torch.zeros(n, device=self._dev), requires_grad=False)
        self.moving_mean = nn.Parameter(torch.zeros(n, device=self._dev), requires_grad=False)
        self.moving_variance = nn.Parameter(torch.ones(n, device=self._dev), requires_grad=False)

    def keras_weights(self):
        return {"dice_alpha": self.alphas, "bn/moving_mean": self.moving_mean,
                "bn/moving_variance": self.moving_variance}

    def set_keras_weights(self, weights, strict=True):
        with torch.no_grad():
            for name, p in self.keras_weights().items():
                if name in weights:
                    p.copy_(torch.as_tensor(weights[name], dtype=torch.float32).reshape(-1))
                elif strict:
                    raise KeyError(name)

    def forward(self, inputs, out=None):
        x = _to_device_f32(inputs, self._dev) if not (torch.is_tensor(inputs) and inputs.is_cuda) else inputs
        if self.alphas is None:
            self.build(x.shape[-1])
        if x.dim() != 2:
            raise NotImplementedError("Dice.forward: 2-D inputs (3-D Dice runs fused in Attention)")
        M, N = x.shape
        if out is None:
            out = torch.empty_like(x)
        call("rs_dice_fwd", ptr(x), x.stride(0), ptr(self.moving_mean), ptr(self.moving_variance),
             self.epsilon, ptr(self.alphas), ptr(out), out.stride(0), M, N, _stream())
        return out


class BatchNormalization(KerasModule):
    """Keras BatchNormalization() at inference (model/din.py:47,89):
    y = x*inv + (beta - mean*inv), inv = gamma*rsqrt(var + eps), eps 1e-3."""

    def __init__(self, epsilon=1e-3, device=None):
        super().__init__(device)
        self.epsilon = float(epsilon)
        self.gamma = self.beta = self.moving_mean = self.moving_variance = None

    def build(self, n):
        d = self._dev
        self.gamma = nn.Parameter(torch.ones(n, device=d), requires_grad=False)
        self.beta = nn.Parameter(torch.zeros(n, device=d), requires_grad=False)
        self.moving_mean = nn.Parameter(torch.zeros(n, device=d), requires_grad=False)
        self.moving_variance = nn.Parameter(torch.ones(n, device=d), requires_grad=False)

    def keras_weights(self):
        return {"gamma": self.gamma, "beta": self.beta, "moving_mean": self.moving_mean,
                "moving_variance": self.moving_variance}

    def set_keras_weights(self, weights, strict=True):
        with torch.no_grad():
            for name, p in self.keras_weights().items():
                p.copy_(torch.as_tensor(weights[name], dtype=torch.float32).reshape(-1))

    def affine(self):
        """(inv, shift) = (gamma rsqrt(var + eps), beta - mean inv), cached per
        parameter version (inference calls launch no elementwise kernels)."""
        def build():
            inv = torch.rsqrt(self.moving_variance + self.epsilon) * self.gamma
            return inv, self.beta - self.moving_mean * inv
        return self._packed("affine", (self.gamma, self.beta, self.moving_mean, self.moving_variance), build)

    def forward(self, x, out=None):
        if self.gamma is None:
            self.build(x.shape[-1])
        inv, shift = self.affine()
        M, N = x.shape
        if out is None:
            out = torch.empty_like(x)
        call("rs_affine_act", ptr(x), x.stride(0), ptr(inv), ptr(shift), None, 0, ptr(out), out.stride(0), M, N,
             _stream())
        return out


# ------------------------------------------------------------ DIN attention
class Attention(KerasModule):
    """Attention(hidden_units, activation='prelu') — layer/interaction.py:355-406.

    'prelu': Dense(h, PReLU()) per hidden unit count; the PReLU sits on a 3-D
    input so its alpha has shape [T, h] (Keras shared_axes=None), built on the
    first call.  'dice': len(hidden_units) Dice layers on the 4k-wide concat and
    NO Dense (exactly as the reference, :363-364).  Then Dense(1).
    ``forward([query[B,k], key[B,T,k], value[B,T,k], mask[B,T]]) -> [B,k]``.
    """

    def __init__(self, hidden_units, activation="prelu", device=None, seed=None):
        super().__init__(device, seed)
        if activation not in ("prelu", "dice"):
            raise ValueError(f"Attention activation must be 'prelu' or 'dice', got {activation!r}")
        self.hidden_units = tuple(int(h) for h in hidden_units)
        self.activation = activation
        self.kernels = nn.ParameterList()
        self.biases = nn.ParameterList()
        self.alphas = nn.ParameterList()
        self.dice = nn.ModuleList()
        self.out_kernel = self.out_bias = None
        self.T = None

    def build(self, T, k):
        self.T = T
        n = 4 * k
        if self.activation == "prelu":
            for h in self.hidden_units:
                self.kernels.append(nn.Parameter(_glorot_uniform(n, h, self._gen, self._dev), requires_grad=False))
                self.biases.append(nn.Parameter(torch.zeros(h, device=self._dev), requires_grad=False))
                self.alphas.append(nn.Parameter(torch.zeros(T, h, device=self._dev), requires_grad=False))
                n = h
        else:
            for _ in self.hidden_units:
                d = Dice(device=self._dev)
                d.build(4 * k)
                self.dice.append(d)
        self.out_kernel = nn.Parameter(_glorot_uniform(n, 1, self._gen, self._dev), requires_grad=False)
        self.out_bias = nn.Parameter(torch.zeros(1, device=self._dev), requires_grad=False)

    def fused_ok(self, k):
        """The one-launch MFMA kernel (rs_din_attention_fwd) takes the shape:
        the reference's two hidden layers, H <= 128, k in {4, 8, 16, 32}.
        Other depths / sizes run the generic path (rs_din_attention_gen_fwd)."""
        return (self.activation == "prelu" and len(self.hidden_units) == 2 and k in (4, 8, 16, 32)
                and max(self.hidden_units) <= 128)

    def ids_ok(self, k):
        """The id-driven fused path (rs_din_attention_ids_fwd) supports it."""
        return (self.activation == "prelu" and self.out_kernel is not None and len(self.hidden_units) == 2
                and k in (4, 8, 16) and self.hidden_units[0] <= 128 and self.hidden_units[1] <= 64)

    def prepared_ids(self, k):
        params = list(self.kernels) + list(self.biases) + list(self.alphas) + [self.out_kernel, self.out_bias]

        def build():
            h1, h2 = self.hidden_units
            prep = sized("rs_din_prepared_size", self.T, k, h1, h2, device=self._dev)
            call("rs_din_prepare", ptr(self.kernels[0]), ptr(self.biases[0]), ptr(self.alphas[0]), h1,
                 ptr(self.kernels[1]), ptr(self.biases[1]), ptr(self.alphas[1]), h2, ptr(self.out_kernel),
                 ptr(self.out_bias), self.T, k, ptr(prep), _stream())
            return prep
        return self._packed("ids", params, build, extra=(k, self.T))

    def forward_ids(self, table, vocab, hist, cand, err=None, out=None, scores=None, cand_out=None):
        """Attention over key = value = table[hist], query = table[cand],
        mask = hist != 0 (model/din.py:56-80) without materialising [B,T,k].
        ``cand_out`` [B, k] (any row stride): also write the candidate rows
        table[cand] there, in the same launch (DIN.call's concat)."""
        B, T = hist.shape
        k = table.shape[1]
        if self.out_kernel is None:
            self.build(T, k)
        if T != self.T:
            raise ValueError(f"Attention built for T={self.T} (PReLU alpha is [T,h]); got T={T}")
        if out is None:
            out = torch.empty(B, k, dtype=torch.float32, device=self._dev)
        if scores is None:
            scores = torch.empty(B, T, dtype=torch.float32, device=self._dev)
        if scores.numel() < B * T:
            raise ValueError("forward_ids: scores workspace needs B*T elements")
        h1, h2 = self.hidden_units
        if cand_out is not None:
            if cand_out.shape != (B, k) or cand_out.stride(1) != 1 or cand_out.dtype != torch.float32:
                raise ValueError("forward_ids: cand_out must be a float32 [B, k] view with unit column stride")
            call("rs_din_attention_ids_cand_fwd", ptr(hist), _lib.id_kind(hist), hist.stride(0), ptr(cand),
                 cand.stride(0), T, k, ptr(table), vocab, h1, h2, ptr(self.prepared_ids(k)), ptr(scores), ptr(out),
                 out.stride(0), ptr(cand_out), cand_out.stride(0), B, ptr(err), _stream())
            return out
        call("rs_din_attention_ids_fwd", ptr(hist), _lib.id_kind(hist), hist.stride(0), ptr(cand),
             cand.stride(0), T, k, ptr(table), vocab, h1, h2, ptr(self.prepared_ids(k)), ptr(scores), ptr(out),
             out.stride(0), B, ptr(err), _stream())
        return out

    def keras_weights(self):
        out = {}
        for i in range(len(self.kernels)):
            out[f"dense_{i}/kernel"] = self.kernels[i]
            out[f"dense_{i}/bias"] = self.biases[i]
            out[f"dense_{i}/prelu/alpha"] = self.alphas[i]
        for i, d in enumerate(self.dice):
            out.update({f"dice_{i}/{k}": v for k, v in d.keras_weights().items()})
        out["out/kernel"] = self.out_kernel
        out["out/bias"] = self.out_bias
        return out

    def set_keras_weights(self, weights, strict=True):
        own = self.keras_weights()
        with torch.no_grad():
            for name, p in own.items():
                if name in weights:
                    p.copy_(torch.as_tensor(weights[name], dtype=torch.float32).reshape(p.shape))
                elif strict:
                    raise KeyError(name)

    def forward(self, inputs, out=None):
        query, key, value, mask = inputs
        q = _to_device_f32(query, self._dev)
        key = _to_device_f32(key, self._dev)
        value = key if value is None else _to_device_f32(value, self._dev)
        mask = _to_device_f32(mask, self._dev)
        q, key, value, mask = (t.contiguous() for t in (q, key, value, mask))  # the kernels take dense rows
        B, T, k = key.shape
        if self.out_kernel is None:
            self.build(T, k)
        if T != self.T and self.activation == "prelu":
            raise ValueError(f"Attention built for T={self.T} (PReLU alpha is [T,h]); got T={T}")
        if out is None:
            out = torch.empty(B, k, dtype=torch.float32, device=self._dev)
        s = _stream()
        if self.activation == "prelu" and not self.fused_ok(k):
            n = len(self.hidden_units)
            hid = ints(self.hidden_units)
            wsz = _lib.lib().rs_din_attention_gen_workspace_size(B, T, k, n, hid)
            if wsz < 0:
                _lib.check(-1, "rs_din_attention_gen_workspace_size")
            ws = scratch(self, "_gen_ws", wsz)
            call("rs_din_attention_gen_fwd", ptr(q), ptr(key), ptr(value), ptr(mask), T, k, n, hid,
                 ptrs(self.kernels), ptrs(self.biases), ptrs(self.alphas),
                 ptr(self.out_kernel), ptr(self.out_bias), ptr(out), B, ptr(ws), ws.numel(), s)
        elif self.activation == "prelu":
            h1, h2 = self.hidden_units
            call("rs_din_attention_fwd", ptr(q), ptr(key), ptr(value), ptr(mask), T, k, ptr(self.kernels[0]),
                 ptr(self.biases[0]), ptr(self.alphas[0]), h1, ptr(self.kernels[1]), ptr(self.biases[1]),
                 ptr(self.alphas[1]), h2, ptr(self.out_kernel), ptr(self.out_bias), ptr(out), B, s)
        else:
            nl = len(self.dice)
            if nl:
                al = torch.stack([d.alphas for d in self.dice]).contiguous()
                mu = torch.stack([d.moving_mean for d in self.dice]).contiguous()
                var = torch.stack([d.moving_variance for d in self.dice]).contiguous()
                eps = self.dice[0].epsilon
            else:
                al = mu = var = None
                eps = 1e-9
            call("rs_din_attention_dice_fwd", ptr(q), ptr(key), ptr(value), ptr(mask), T, k, nl, ptr(al), ptr(mu),
                 ptr(var), eps, ptr(self.out_kernel), ptr(self.out_bias), ptr(out), B, s)
        return out


def sigmoid_combine(a, b=None, c0=1.0, c1=1.0, out=None):
    """out = sigmoid(c0*a + c1*b) elementwise (model heads)."""
    if out is None:
        out = torch.empty_like(a)
    call("rs_sigmoid_combine", ptr(a), ptr(b), float(c0), float(c1), ptr(out), a.numel(), _stream())
    return out


# ------------------------------------ other interactions
class InteractionLayer(KerasModule):
    """InteractionLayer() — layer/interaction.py:280-297: [B,F,k] -> [B,P,k]
    element-wise products of the (i<j) row-major field pairs
    (rs_pair_products_fwd)."""

    def __init__(self, device=None):
        super().__init__(device)

    def forward(self, inputs, out=None):
        e = _to_device_f32(inputs, self._dev).contiguous()
        B, F, k = e.shape
        P = F * (F - 1) // 2
        if out is None:
            out = torch.empty(B, P, k, dtype=torch.float32, device=self._dev)
        call("rs_pair_products_fwd", ptr(e), F * k, F, k, B, ptr(out), _stream())
        return out


class AttentionLayer(KerasModule):
    """AttentionLayer() — layer/interaction.py:300-319.  Holds the reference's
    weights (attention_w = Dense(n_rows, relu), attention_h = Dense(1)) for
    Keras-name weight exchange; its softmax runs over a size-1 axis, so every
    score is exactly 1 and the output is the sum over the rows
    (rs_attention_pool_fwd) — the weights cannot change the result."""

    def __init__(self, device=None, seed=None):
        super().__init__(device, seed)
        self.attention_w = self.attention_h = None

    def build(self, n_rows, k):
        self.attention_w = Dense(n_rows, activation="relu", device=self._dev, seed=_subseed(self._gen),
                                 input_dim=k)
        self.attention_h = Dense(1, device=self._dev, seed=_subseed(self._gen), input_dim=n_rows)

    def keras_weights(self):
        if self.attention_w is None:
            return {}
        out = {f"dense/{n}": v for n, v in self.attention_w.keras_weights().items()}
        out.update({f"dense_1/{n}": v for n, v in self.attention_h.keras_weights().items()})
        return out

    def set_keras_weights(self, weights, strict=True):
        self.attention_w.set_keras_weights({n[6:]: v for n, v in weights.items() if n.startswith("dense/")}, strict)
        self.attention_h.set_keras_weights({n[8:]: v for n, v in weights.items() if n.startswith("dense_1/")},
                                           strict)

    def forward(self, inputs, out=None):
        x = _to_device_f32(inputs, self._dev).contiguous()
        B, P, k = x.shape
        if self.attention_w is None:
            self.build(P, k)
        if out is None:
            out = torch.empty(B, k, dtype=torch.float32, device=self._dev)
        call("rs_attention_pool_fwd", ptr(x), P * k, P, k, B, ptr(out), _stream())
        return out


_AFM_MODES = {"att": 0, "avg": 1, "max": 2}


class AFMLayer(KerasModule):
    """AFMLayer(feature_columns, mode) — layer/interaction.py:322-351:
    per-field Embedding(feat_onehot_dim, embed_dim) -> InteractionLayer ->
    'avg' mean / 'max' max / attention (== sum) over the pairs -> Dense(1) ->
    sigmoid.  ids -> rows -> pooled pairs -> head in ONE launch
    (rs_embed_pair_pool_fwd); the [B,P,k] pair tensor is never formed."""

    def __init__(self, feature_columns, mode, device=None, seed=None):
        super().__init__(device, seed)
        self.dense_feature_columns, self.sparse_feature_columns = feature_columns
        self.mode = mode
        dims = {int(f["embed_dim"]) for f in self.sparse_feature_columns}
        if len(dims) != 1:
            raise ValueError("AFMLayer: every sparse feature needs the same embed_dim (the pairs are stacked)")
        self.k = dims.pop()
        self.nd = len(self.dense_feature_columns)
        self.embed_layer = EmbedLayer(self.sparse_feature_columns, self.k, device=device, seed=_subseed(self._gen))
        self.interaction_layer = InteractionLayer(device=device)
        F = self.embed_layer.n_fields
        self.attention_layer = None
        if mode == "att":
            self.attention_layer = AttentionLayer(device=device, seed=_subseed(self._gen))
            self.attention_layer.build(F * (F - 1) // 2, self.k)
        self.output_layer = Dense(1, device=device, seed=_subseed(self._gen), input_dim=self.k)
        self._err = _ErrFlag(self._dev)

    def pooled(self, inputs, check_ids=True, n_sigmoid=1):
        """(pooled [B,k], head [B,1] = sigmoid^n_sigmoid(Dense(1)(pooled)))."""
        if isinstance(inputs, (tuple, list)):
            ids = _ids_tensor(inputs[1], self._dev)
        else:
            ids = _to_device_f32(inputs, self._dev)[:, self.nd:]
        B = ids.shape[0]
        e = self.embed_layer
        pooled = torch.empty(B, self.k, dtype=torch.float32, device=self._dev)
        head = torch.empty(B, 1, dtype=torch.float32, device=self._dev)
        call("rs_embed_pair_pool_fwd", ptr(ids), _lib.id_kind(ids), ids.stride(0), ptr(e.table),
             ptr(e.field_offsets), ptr(e.field_vocab), e.n_fields, self.k, _AFM_MODES.get(self.mode, 0), None, 0, 0,
             ptr(pooled), self.k, 0, ptr(self.output_layer.kernel), ptr(self.output_layer.bias), n_sigmoid,
             ptr(head), B, ptr(self._err.t), _stream())
        if check_ids:
            self._err.check("AFMLayer")
        return pooled, head

    def forward(self, inputs, check_ids=True):
        return self.pooled(inputs, check_ids, n_sigmoid=1)[1]


class FFMLayer(KerasModule):
    """FFMLayer(feature_columns, k, w_reg=1e-4, v_reg=1e-4) —
    layer/interaction.py:117-163.  Weights in Keras shapes: w0 (1,), w
    (feature_num, 1), v (feature_num, field_num, k), feature_num = nd +
    sum(feat_onehot_dim), field_num = nd + F.  ``forward(X[B, nd+F])`` on
    label-encoded ids: the one-hot x is never formed — row nd + offset_c + id
    of w and v is gathered (rs_ffm_fwd, one wave per sample)."""

    def __init__(self, feature_columns, k, w_reg=1e-4, v_reg=1e-4, device=None, seed=None):
        super().__init__(device, seed)
        self.dense_feature_columns, self.sparse_feature_columns = feature_columns
        self.k = int(k)
        self.w_reg, self.v_reg = w_reg, v_reg
        self.nd = len(self.dense_feature_columns)
        self.onehot_dims = [int(f["feat_onehot_dim"]) for f in self.sparse_feature_columns]
        self.feature_num = sum(self.onehot_dims) + self.nd
        self.field_num = self.nd + len(self.sparse_feature_columns)
        offs = [0]
        for v in self.onehot_dims[:-1]:
            offs.append(offs[-1] + v)
        dev = self._dev
        self.register_buffer("field_offsets", torch.tensor(offs, dtype=torch.int64, device=dev))
        self.register_buffer("field_vocab", torch.tensor(self.onehot_dims, dtype=torch.int64, device=dev))
        self.w0 = nn.Parameter(torch.zeros(1, device=dev), requires_grad=False)
        self.w = nn.Parameter(_normal((self.feature_num, 1), self._gen, dev), requires_grad=False)
        v = torch.empty(self.feature_num, self.field_num, self.k, dtype=torch.float32, device=dev)
        if v.is_cuda:
            g = torch.Generator(device=v.device)
            g.manual_seed(_subseed(self._gen))
            v.normal_(0.0, 0.05, generator=g)
        else:
            v.normal_(0.0, 0.05, generator=self._gen)
        self.v = nn.Parameter(v, requires_grad=False)
        self._err = _ErrFlag(dev)

    def keras_weights(self):
        return {"w0": self.w0, "w": self.w, "v": self.v}

    def set_keras_weights(self, weights, strict=True):
        with torch.no_grad():
            for name, p in self.keras_weights().items():
                p.copy_(torch.as_tensor(weights[name], dtype=torch.float32).reshape(p.shape))

    def logits(self, inputs, n_sigmoid=0):
        if isinstance(inputs, (tuple, list)):
            dense, ids = _to_device_f32(inputs[0], self._dev), _ids_tensor(inputs[1], self._dev)
        else:
            X = _to_device_f32(inputs, self._dev)
            dense, ids = X[:, :self.nd], X[:, self.nd:]
        B = ids.shape[0]
        out = torch.empty(B, 1, dtype=torch.float32, device=self._dev)
        # tf.one_hot (layer/interaction.py:145-146) maps an out-of-range id to
        # a zero row without an error: the kernel does the same (no check)
        call("rs_ffm_fwd", ptr(ids), _lib.id_kind(ids), ids.stride(0), ptr(dense), dense.stride(0), self.nd,
             ptr(self.v), ptr(self.w), ptr(self.w0), ptr(self.field_offsets), ptr(self.field_vocab),
             len(self.onehot_dims), self.k, n_sigmoid, ptr(out), B, None, _stream())
        return out

    def forward(self, inputs):
        return self.logits(inputs, 0)


# ------------------------------------------------- DeepCrossing / Wide&Deep
_RES_MAXH, _RES_MAXU = 4, 16  # res_tower.hip RES_MAXH / RES_MAXU


def _res_ok(d, hidden, n_units):
    return bool(_lib.lib().rs_res_tower_ok(int(d), len(hidden), ints(hidden), int(n_units)))


def _res_prepare(units, head, device):
    """The packed image (rs_res_tower_prepare) of a stack of built ResLayers
    with equal widths, optionally with the model's Dense(1) head."""
    d, hidden = units[0].input_dim, units[0].hidden_units
    nh, nu = len(hidden), len(units)
    ci = ints(hidden)
    prep = sized("rs_res_tower_prepared_size", d, nh, ci, nu, 1 if head is not None else 0, device=device)
    layers = [l for u in units for l in u._layers()]
    call("rs_res_tower_prepare", d, nh, ci, nu, ptrs([l.kernel for l in layers]), ptrs([l.bias for l in layers]),
         ptr(head.kernel) if head is not None else None, ptr(head.bias) if head is not None else None, ptr(prep),
         _stream())
    return prep


def _res_params(layers):
    return [p for l in layers for p in (l.kernel, l.bias)]


class ResLayer(KerasModule):
    """ResLayer(hidden_units) — layer/interaction.py:261-278: h = x through
    Dense(u, relu) per hidden width, then a linear Dense(d) (built from the
    input width on the first call or by ``build(d)``); relu(x + h).

    ``forward(x[B, d])`` is ONE rs_res_tower_fwd launch (res_tower.hip: the
    tile stays in LDS, the skip operand in registers) when the shape is
    supported and x is a device tensor with contiguous rows; otherwise
    rs_dense_fwd per layer plus a torch add / relu."""

    def __init__(self, hidden_units, device=None, seed=None):
        super().__init__(device, seed)
        self.hidden_units = [int(u) for u in hidden_units]
        self.dense_layer = nn.ModuleList(
            [Dense(u, activation="relu", device=device, seed=_subseed(self._gen)) for u in self.hidden_units])
        self._out_seed = _subseed(self._gen)
        self.output_layer = None
        self.input_dim = None

    @property
    def built(self):
        return self.output_layer is not None

    def build(self, d):
        d = int(d)
        n = d
        for layer in self.dense_layer:
            layer.build(n)
            n = layer.units
        self.output_layer = Dense(d, activation=None, device=self._dev, seed=self._out_seed, input_dim=n)
        self.input_dim = d
        self._invalidate()

    def _layers(self):
        return list(self.dense_layer) + [self.output_layer]

    def keras_weights(self):
        if not self.built:
            raise RuntimeError("ResLayer: not built (call build(d) or run a forward first)")
        out = {}
        for i, l in enumerate(self.dense_layer):
            out[f"dense_{i}/kernel"], out[f"dense_{i}/bias"] = l.kernel, l.bias
        out["dense_out/kernel"], out["dense_out/bias"] = self.output_layer.kernel, self.output_layer.bias
        return out

    def set_keras_weights(self, weights, strict=True):
        own = self.keras_weights()
        if strict and set(own) != set(weights):
            raise KeyError(f"ResLayer: expected weights {sorted(own)}, got {sorted(weights)}")
        with torch.no_grad():
            for name, p in own.items():
                if name in weights:
                    p.copy_(torch.as_tensor(weights[name], dtype=torch.float32).reshape(p.shape))
        self._invalidate()

    def tower_ok(self):
        return self.built and len(self.hidden_units) >= 1 and _res_ok(self.input_dim, self.hidden_units, 1)

    def prepared(self):
        """Weights packed for rs_res_tower_fwd, cached until a weight changes."""
        return self._packed("res", _res_params(self._layers()), lambda: _res_prepare([self], None, self._dev))

    def forward_layers(self, x):
        """The per-layer composition: rs_dense_fwd per Dense, torch add / relu."""
        h = x
        for layer in self._layers():
            h = layer(h)
        return torch.relu(x + h)

    def forward(self, inputs):
        x = inputs if (torch.is_tensor(inputs) and inputs.is_cuda and inputs.dtype == torch.float32) \
            else _to_device_f32(inputs, self._dev)
        if not self.built:
            self.build(x.shape[-1])
        B, d = x.shape
        if d != self.input_dim:
            raise ValueError(f"ResLayer built for {self.input_dim} inputs, got {d}")
        if not (x.is_cuda and x.stride(1) == 1 and self.tower_ok()):
            return self.forward_layers(x)
        out = torch.empty(B, d, dtype=torch.float32, device=self._dev)
        nh = len(self.hidden_units)
        call("rs_res_tower_fwd", ptr(x), x.stride(0), d, nh, ints(self.hidden_units), 1,
             ptr(self.prepared()), 0, ptr(out), out.stride(0), B, _stream())
        return out


_MMOE_MAXL = 4  # mmoe.hip MMOE_MAXL (tower layers, the output Dense included)


def _mmoe_dims(hidden, towers):
    """tower_dims of the rs_mmoe_* entries: [H] alone for the layer-only form."""
    return [int(hidden)] + ([l.units for l in towers[0]._layers()] if towers else [])


def _mmoe_ok(d, hidden, n_experts, n_tasks, dims):
    return bool(_lib.lib().rs_mmoe_ok(int(d), int(hidden), int(n_experts), int(n_tasks), len(dims) - 1, ints(dims)))


def _mmoe_params(layer, towers):
    ps = [layer.expert_matrix, layer.expert_bias] + layer.gate_matrix + (layer.gate_bias or [])
    ps += [p for tw in towers for l in tw._layers() for p in (l.kernel, l.bias)]
    return [p for p in ps if p is not None]


def _mmoe_prepare(layer, towers, device):
    """The packed image (rs_mmoe_prepare) of a built mmoe_layer, alone or with
    one tower_layer per task (equal widths)."""
    d, H, E, T = layer.input_dim, layer.hidden_units, layer.num_experts, layer.num_tasks
    dims = _mmoe_dims(H, towers)
    L = len(dims) - 1
    ci = ints(dims)
    prep = sized("rs_mmoe_prepared_size", d, H, E, T, L, ci, device=device)
    tl = [l for tw in towers for l in tw._layers()]
    call("rs_mmoe_prepare", d, H, E, T, ptr(layer.expert_matrix), ptr(layer.expert_bias), ptrs(layer.gate_matrix),
         ptrs(layer.gate_bias) if layer.gate_bias else None, L, ci, ptrs([l.kernel for l in tl]) if tl else None,
         ptrs([l.bias for l in tl]) if tl else None, ptr(prep), _stream())
    return prep


def _mmoe_input(inputs, layer):
    """The float32 input rows [B, d] (contiguous columns) of a built-on-demand
    mmoe_layer."""
    x = inputs if (torch.is_tensor(inputs) and inputs.is_cuda and inputs.dtype == torch.float32) \
        else _to_device_f32(inputs, layer._dev)
    if x.dim() != 2:
        raise ValueError(f"mmoe_layer: expected a [batch, features] matrix, got shape {tuple(x.shape)}")
    if x.stride(1) != 1:
        x = x.contiguous()
    if not layer.built:
        layer.build(x.shape[-1])
    if x.shape[1] != layer.input_dim:
        raise ValueError(f"mmoe_layer built for {layer.input_dim} inputs, got {x.shape[1]}")
    return x


class mmoe_layer(KerasModule):
    """mmoe_layer(hidden_units, num_experts, num_tasks, use_expert_bias=True,
    use_gate_bias=True) — layer/interaction.py:429-509: num_experts experts
    relu(x @ expert_matrix[:, :, e] + expert_bias[:, e]), per task a gate
    softmax(x @ gate_matrix{t} + gate_bias{t}) over the experts, and the gated
    sum: ``forward(x[B, d])`` returns num_tasks tensors [B, hidden_units], views
    of one [B, num_tasks * hidden_units] buffer.

    Weights (built from the input width on the first call or by ``build(d)``),
    all random_normal N(0, 0.05) as in the reference: ``expert_matrix``
    [d, H, E], ``expert_bias`` [H, E], ``gate_matrix{t}`` [d, E],
    ``gate_bias{t}`` [E].

    The forward is ONE rs_mmoe_fwd launch without towers (mmoe.hip) when
    ``fused_ok()``; otherwise ``forward_unfused``: rs_dense_fwd for the
    experts, one per gate, torch softmax / multiply / sum."""

    def __init__(self, hidden_units, num_experts, num_tasks, use_expert_bias=True, use_gate_bias=True, device=None,
                 seed=None, input_dim=None):
        super().__init__(device, seed)
        self.hidden_units, self.num_experts, self.num_tasks = int(hidden_units), int(num_experts), int(num_tasks)
        if min(self.hidden_units, self.num_experts, self.num_tasks) < 1:
            raise ValueError("mmoe_layer: hidden_units, num_experts and num_tasks must be >= 1")
        self.use_expert_bias, self.use_gate_bias = bool(use_expert_bias), bool(use_gate_bias)
        self.expert_matrix = self.expert_bias = None
        self.input_dim = None
        if input_dim is not None:
            self.build(input_dim)

    @property
    def built(self):
        return self.expert_matrix is not None

    def build(self, d):
        d, H, E = int(d), self.hidden_units, self.num_experts
        new = lambda *shape: nn.Parameter(_normal(shape, self._gen, self._dev), requires_grad=False)
        self.expert_matrix = new(d, H, E)
        if self.use_expert_bias:
            self.expert_bias = new(H, E)
        for t in range(self.num_tasks):
            setattr(self, f"gate_matrix{t}", new(d, E))
        if self.use_gate_bias:
            for t in range(self.num_tasks):
                setattr(self, f"gate_bias{t}", new(E))
        self.input_dim = d
        self._invalidate()

    @property
    def gate_matrix(self):
        return [getattr(self, f"gate_matrix{t}") for t in range(self.num_tasks)]

    @property
    def gate_bias(self):
        return [getattr(self, f"gate_bias{t}") for t in range(self.num_tasks)] if self.use_gate_bias else None

    def keras_weights(self):
        if not self.built:
            raise RuntimeError("mmoe_layer: not built (call build(d) or run a forward first)")
        return super().keras_weights()

    def fused_ok(self):
        H = self.hidden_units
        return self.built and _mmoe_ok(self.input_dim, H, self.num_experts, self.num_tasks, [H])

    def prepared(self):
        """Weights packed for rs_mmoe_fwd without towers, cached until a weight changes."""
        return self._packed("mmoe", _mmoe_params(self, []), lambda: _mmoe_prepare(self, [], self._dev))

    def forward_fused(self, x):
        """mmoe_layer.call as one launch: the mixes [B, T * H]."""
        B, d = x.shape
        H, E, T = self.hidden_units, self.num_experts, self.num_tasks
        mix = torch.empty(B, T * H, dtype=torch.float32, device=self._dev)
        call("rs_mmoe_fwd", ptr(x), x.stride(0), d, H, E, T, 0, ints([H]), None, ptr(self.prepared()), ptr(mix),
             mix.stride(0), None, 0, 0, B, _stream())
        return mix

    def forward_unfused(self, x):
        """The composition from the older entries: the mixes [B, T * H]."""
        B, d = x.shape
        H, E, T = self.hidden_units, self.num_experts, self.num_tasks
        mix = torch.empty(B, T * H, dtype=torch.float32, device=self._dev)
        if B == 0:
            return mix
        experts = torch.empty(B, H * E, dtype=torch.float32, device=self._dev)
        call("rs_dense_fwd", ptr(x), x.stride(0), ptr(self.expert_matrix), ptr(self.expert_bias), None,
             _lib.ACT["relu"], ptr(experts), experts.stride(0), B, d, H * E, _stream())
        experts = experts.view(B, H, E)
        gb = self.gate_bias
        for t, gm in enumerate(self.gate_matrix):
            logits = torch.empty(B, E, dtype=torch.float32, device=self._dev)
            call("rs_dense_fwd", ptr(x), x.stride(0), ptr(gm), ptr(gb[t]) if gb else None, None, 0, ptr(logits),
                 logits.stride(0), B, d, E, _stream())
            gate = torch.softmax(logits, dim=-1)
            mix[:, t * H:(t + 1) * H] = (experts * gate.unsqueeze(1)).sum(-1)
        return mix

    def forward(self, inputs):
        x = _mmoe_input(inputs, self)
        mix = self.forward_fused(x) if self.fused_ok() else self.forward_unfused(x)
        H = self.hidden_units
        return [mix[:, t * H:(t + 1) * H] for t in range(self.num_tasks)]


class tower_layer(DNNLayer):
    """tower_layer(hidden_units, output_dim, activation='relu') —
    layer/interaction.py:512-523: DNNLayer without the Dropout (same weight
    names, dense_{i}/… and dense_out/…).  (The reference's __init__ assigns its
    sub-layers before super().__init__(), the reverse of the order Keras asks
    for; recorded in DESIGN.md, not imitated and not "fixed" there.)"""

    def __init__(self, hidden_units, output_dim, activation="relu", device=None, seed=None, input_dim=None):
        super().__init__(hidden_units, output_dim, activation, dropout=0.0, device=device, seed=seed)
        if input_dim is not None:
            self.build(input_dim)


class WideLayer(KerasModule):
    """WideLayer() — layer/interaction.py:11-26: w0 + x @ w with w0 (1,)
    zeros and w (n, 1) ~ N(0, 0.05), built from the input width on the first
    call.  ``forward(x[B, n])`` is rs_dense_fwd with one output unit (w0 as
    its bias).  ``forward_onehot(dense, ids, field_offsets, field_widths)``
    takes the compact form of Wide&Deep's wide input [dense | dense | one-hot]
    (model/wideDeep.py:22-27) and gathers one scalar of w per field
    (rs_wide_onehot_fwd) instead of multiplying by zeros."""

    def __init__(self, device=None, seed=None, w_reg=1e-4):
        super().__init__(device, seed)
        self.w_reg = float(w_reg)  # l2 on w (layer/interaction.py:22); training only
        self.w0 = self.w = None

    @property
    def built(self):
        return self.w is not None

    def build(self, n):
        self.w0 = nn.Parameter(torch.zeros(1, device=self._dev), requires_grad=False)
        self.w = nn.Parameter(_normal((int(n), 1), self._gen, self._dev), requires_grad=False)

    def keras_weights(self):
        if not self.built:
            raise RuntimeError("WideLayer: not built (call build(n) or run a forward first)")
        return {"w0": self.w0, "w": self.w}

    def set_keras_weights(self, weights, strict=True):
        own = self.keras_weights()
        if strict and set(own) != set(weights):
            raise KeyError(f"WideLayer: expected weights {sorted(own)}, got {sorted(weights)}")
        with torch.no_grad():
            for name, p in own.items():
                if name in weights:
                    p.copy_(torch.as_tensor(weights[name], dtype=torch.float32).reshape(p.shape))

    def forward(self, inputs):
        x = inputs if (torch.is_tensor(inputs) and inputs.is_cuda and inputs.dtype == torch.float32) \
            else _to_device_f32(inputs, self._dev)
        if not self.built:
            self.build(x.shape[-1])
        B, n = x.shape
        if n != self.w.shape[0]:
            raise ValueError(f"WideLayer built for {self.w.shape[0]} inputs, got {n}")
        out = torch.empty(B, 1, dtype=torch.float32, device=self._dev)
        call("rs_dense_fwd", ptr(x), x.stride(0), ptr(self.w), ptr(self.w0), None, 0, ptr(out), 1, B, n, 1,
             _stream())
        return out

    def forward_onehot(self, dense, ids, field_offsets, field_widths, check_ids=True):
        ids = _ids_tensor(ids, self._dev)
        B, F = ids.shape
        offs = torch.as_tensor(field_offsets, dtype=torch.int64).to(self._dev)
        wid = torch.as_tensor(field_widths, dtype=torch.int64).to(self._dev)
        if dense is None:
            nd = 0
        else:
            dense = _to_device_f32(dense, self._dev)
            nd = dense.shape[1]
        if offs.numel() != F or wid.numel() != F:
            raise ValueError(f"WideLayer: {F} id columns need {F} field offsets and widths")
        n = 2 * nd + int(wid.sum())  # (a host sum: not inside a graph capture)
        if not self.built:
            self.build(n)
        if n != self.w.shape[0]:
            raise ValueError(f"WideLayer built for {self.w.shape[0]} inputs, got 2*{nd} + {n - 2 * nd}")
        out = torch.empty(B, 1, dtype=torch.float32, device=self._dev)
        err = _ErrFlag(self._dev)
        call("rs_wide_onehot_fwd", ptr(ids), _lib.id_kind(ids), ids.stride(0), ptr(dense) if nd else None,
             dense.stride(0) if nd else 0, nd, ptr(offs), ptr(wid), F, ptr(self.w), ptr(self.w0), ptr(out), B,
             ptr(err.t), _stream())
        if check_ids:
            err.check("WideLayer")
        return out


# ------------------------------------------------- DIEN: sequence layers
_DIEN_ACTS = {"relu": 1, "sigmoid": 3, "dice": 4}  # RS_ACT_RELU, RS_ACT_SIGMOID, RS_ACT_DICE
_DIEN_UPDATES = {"reference": 0, "paper": 1}
_RNN_MAXW = 64  # dien.hip: input width and units of rs_gru_fwd / rs_augru_fwd, D of the fused launch


def _glorot_normal(fan_in, fan_out, gen, device):
    """Keras glorot_normal: a normal truncated at two standard deviations,
    scaled so that the truncated variable has variance 2 / (fan_in + fan_out)."""
    std = math.sqrt(2.0 / (fan_in + fan_out)) / 0.87962566103423978
    t = torch.randn(fan_in, fan_out, generator=gen, device="cpu")
    for _ in range(64):
        far = t.abs() > 2
        if not bool(far.any()):
            break
        t[far] = torch.randn(int(far.sum()), generator=gen, device="cpu")
    return t.clamp_(-2, 2).mul_(std).to(device)


def _orthogonal(rows, cols, gen, device):
    """Keras Orthogonal(gain=1): Q of the QR of a normal matrix, signs fixed by diag(R)."""
    a = torch.randn(max(rows, cols), min(rows, cols), generator=gen, device="cpu", dtype=torch.float64)
    q, r = torch.linalg.qr(a)
    q = q * torch.sign(torch.diagonal(r))
    if rows < cols:
        q = q.t()
    return q.to(torch.float32).contiguous().to(device)


def _seq_input(x, device, what):
    x = x if (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32) else _to_device_f32(x, device)
    if x.dim() != 3:
        raise ValueError(f"{what}: expected [batch, T, width], got shape {tuple(x.shape)}")
    return x if x.stride(2) == 1 else x.contiguous()


def _lengths(seq_length, device, B):
    t = torch.as_tensor(seq_length)
    if t.dtype not in (torch.int32, torch.int64):
        t = t.to(torch.int64)
    t = t.reshape(-1).to(device).contiguous()
    if t.numel() != B:
        raise ValueError(f"seq_length holds {t.numel()} lengths for a batch of {B}")
    return t


class _Recurrent(KerasModule):
    """kernel [din, 3 units] and recurrent_kernel [units, 3 units], gate order
    z r h, and their packed image (rs_gru_prepare), cached per weight version."""

    use_bias = False

    def __init__(self, units, device=None, seed=None, input_dim=None):
        super().__init__(device, seed)
        self.units = int(units)
        if self.units < 1:
            raise ValueError("units must be >= 1")
        self.kernel = self.recurrent_kernel = self.bias = None
        if input_dim is not None:
            self.build(input_dim)

    @property
    def built(self):
        return self.kernel is not None

    def _recurrent_init(self):
        u = self.units
        return _glorot_uniform(u, 3 * u, self._gen, self._dev)

    def build(self, din):
        din, u = int(din), self.units
        if max(din, u) > _RNN_MAXW:
            raise NotImplementedError(f"{type(self).__name__}: input width and units up to {_RNN_MAXW} "
                                      f"(got {din}, {u})")
        self.input_dim = din
        self.kernel = nn.Parameter(_glorot_uniform(din, 3 * u, self._gen, self._dev), requires_grad=False)
        self.recurrent_kernel = nn.Parameter(self._recurrent_init(), requires_grad=False)
        if self.use_bias:
            self.bias = nn.Parameter(torch.zeros(2, 3 * u, device=self._dev), requires_grad=False)
        self._invalidate()

    def keras_weights(self):
        if not self.built:
            raise RuntimeError(f"{type(self).__name__}: not built (call build(input_dim) or run a forward first)")
        return super().keras_weights()

    def prepared(self):
        ps = [p for p in (self.kernel, self.recurrent_kernel, self.bias) if p is not None]

        def build():
            prep = sized("rs_gru_prepared_size", self.input_dim, self.units, device=self._dev)
            call("rs_gru_prepare", self.input_dim, self.units, ptr(self.kernel), ptr(self.recurrent_kernel),
                 ptr(self.bias), ptr(prep), _stream())
            return prep
        return self._packed("rnn", ps, build)

    def prepared_bwd(self):
        """The transposed recurrent kernel packed for rs_gru_bwd / rs_augru_bwd
        (rs_gru_prepare_bwd), cached per weight version."""
        def build():
            prep = sized("rs_gru_bwd_prepared_size", self.units, device=self._dev)
            call("rs_gru_prepare_bwd", self.units, ptr(self.recurrent_kernel), ptr(prep), _stream())
            return prep
        return self._packed("rnn_bwd", (self.recurrent_kernel,), build)

    def _input(self, inputs):
        x = _seq_input(inputs, self._dev, type(self).__name__)
        if not self.built:
            self.build(x.shape[2])
        if x.shape[2] != self.input_dim:
            raise ValueError(f"{type(self).__name__} built for {self.input_dim} inputs, got {x.shape[2]}")
        return x


class GRU(_Recurrent):
    """GRU(units, return_sequences=False) — the subset of Keras GRU that DIEN
    uses (model/dien.py:65): TF2 defaults reset_after=True, use_bias=True, tanh /
    sigmoid, gate order z r h, zero initial state, no mask.  Weights: ``kernel``
    [din, 3 units] glorot-uniform, ``recurrent_kernel`` [units, 3 units]
    orthogonal, ``bias`` [2, 3 units] zeros (input row, recurrent row).
    ``forward(x[B, T, din])`` is one rs_gru_fwd launch (dien.hip): [B, T, units]
    with return_sequences, else the last state [B, units]."""

    use_bias = True

    def __init__(self, units, return_sequences=False, device=None, seed=None, input_dim=None):
        super().__init__(units, device, seed, input_dim)
        self.return_sequences = bool(return_sequences)

    def _recurrent_init(self):
        return _orthogonal(self.units, 3 * self.units, self._gen, self._dev)

    def forward(self, inputs):
        x = self._input(inputs)
        B, T, _ = x.shape
        u = self.units
        if T < 1:
            raise ValueError("GRU: an empty sequence")
        if self.return_sequences:
            seq = torch.empty(B, T, u, dtype=torch.float32, device=self._dev)
            call("rs_gru_fwd", ptr(x), x.stride(0), x.stride(1), T, self.input_dim, u, ptr(self.prepared()), ptr(seq),
                 None, 0, B, _stream())
            return seq
        last = torch.empty(B, u, dtype=torch.float32, device=self._dev)
        call("rs_gru_fwd", ptr(x), x.stride(0), x.stride(1), T, self.input_dim, u, ptr(self.prepared()), None,
             ptr(last), last.stride(0), B, _stream())
        return last

    def train_forward(self, inputs):
        """(seq [B, T, units], saved): the forward of a training step
        (rs_gru_train_fwd; seq bit-identical to forward's)."""
        return _train_ops.gru_train_forward(self, inputs, _stream())

    def backward(self, x, saved, dseq=None, dlast=None, d_in=True):
        """(dx, dkernel, drecurrent_kernel, dbias) from the gradient of the
        sequence [B, T, units] and / or of the last state [B, units]
        (rs_gru_bwd, then rs_gemm / rs_col_sum_split)."""
        return _train_ops.gru_backward(self, self._input(x), saved, dseq, dlast, _stream(), d_in)


class AUGRUCell(_Recurrent):
    """AUGRUCell(units) — layer/activation.py:91-142: the weights of the
    attention-update GRU, ``kernel`` [din, 3 units] and ``recurrent_kernel``
    [units, 3 units] (add_weight's default glorot-uniform, no bias)."""


class AUGRU(KerasModule):
    """AUGRU(units, gru_type='AUGRU', return_sequences=False) —
    layer/sequence.py:293-395 over AUGRUCell: z = a hsig(x W_z + h U_z),
    r = hsig(x W_r + h U_r), hh = tanh(x W_h + (r h) U_h), h <- z h + (1 - z) hh
    with hsig = clip(0.2 x + 0.5, 0, 1) and a the attention score of the step.
    ``forward(x[B, T, din], att_score[B, T])`` returns the last state [B, units]
    (one rs_augru_fwd launch).  ``gru_type`` is accepted and ignored, as in the
    reference (its __init__ never passes it to the cell).  ``augru_update=
    'paper'`` swaps the blend to the DIEN paper's h <- (1 - z) h + z hh."""

    def __init__(self, units, gru_type="AUGRU", return_sequences=False, augru_update="reference", device=None,
                 seed=None, input_dim=None):
        super().__init__(device, seed)
        if return_sequences:
            raise NotImplementedError("AUGRU: return_sequences=True is not built (DIEN uses the last state)")
        if augru_update not in _DIEN_UPDATES:
            raise ValueError(f"augru_update must be 'reference' or 'paper', got {augru_update!r}")
        self.gru_type, self.augru_update = gru_type, augru_update
        self.cell = AUGRUCell(units, device=device, seed=_subseed(self._gen), input_dim=input_dim)

    @property
    def units(self):
        return self.cell.units

    def keras_weights(self):
        return self.cell.keras_weights()

    def set_keras_weights(self, weights, strict=True):
        self.cell.set_keras_weights(weights, strict)

    def forward(self, inputs, att_score):
        c = self.cell
        x = c._input(inputs)
        B, T, _ = x.shape
        a = att_score if (torch.is_tensor(att_score) and att_score.is_cuda) else _to_device_f32(att_score, self._dev)
        a = a.reshape(B, T).to(torch.float32).contiguous()
        last = torch.empty(B, c.units, dtype=torch.float32, device=self._dev)
        call("rs_augru_fwd", ptr(x), x.stride(0), x.stride(1), ptr(a), a.stride(0), T, c.input_dim, c.units,
             _DIEN_UPDATES[self.augru_update], ptr(c.prepared()), ptr(last), last.stride(0), B, _stream())
        return last

    def train_forward(self, inputs, att_score):
        """(last [B, units], saved) (rs_augru_train_fwd; last bit-identical to forward's)."""
        a = att_score if (torch.is_tensor(att_score) and att_score.is_cuda) else _to_device_f32(att_score, self._dev)
        return _train_ops.augru_train_forward(self, inputs, a, _stream())

    def backward(self, x, att_score, seq_length, saved, dlast, weight_normalization=False, want_da=False):
        """(dx, ds, da, dkernel, drecurrent_kernel) from the gradient of the
        last state.  ``att_score`` [B, T] are the masked (and, with
        weight_normalization, softmax-normalised) scores the forward took and
        ``seq_length`` [B] their mask: ds is the gradient of the scores before
        the mask, da (want_da) that of att_score itself."""
        x = self.cell._input(x)
        L = _lengths(seq_length, self._dev, x.shape[0])
        return _train_ops.augru_backward(self, x, att_score, L, weight_normalization, saved, dlast, _stream(), want_da)


class DNN(KerasModule):
    """DNN(hidden_units, activation='relu', l2_reg=0, dropout_rate=0,
    use_bn=False, output_activation=None) — layer/core.py:123-205 (the
    DeepCTR-style tower; DNNLayer is the reference's other one): per layer
    Dense with bias, BatchNormalization when use_bn, the activation ('relu',
    'sigmoid', 'dice', 'prelu', 'linear' / None) — the last layer included —
    and an inference-inactive Dropout.  Weights ``kernel{i}`` glorot-normal,
    ``bias{i}`` zeros, ``bn{i}/…``, ``dice{i}/…``, ``alpha{i}``.  The input's
    last axis is contracted; leading axes are kept.  Each layer is rs_dense_fwd
    (+ rs_affine_act for BN, rs_dice_fwd for Dice); the models fuse a BN-free
    relu / sigmoid tower into one rs_mlp_fwd launch."""

    def __init__(self, hidden_units, activation="relu", l2_reg=0, dropout_rate=0, use_bn=False,
                 output_activation=None, device=None, seed=None, input_dim=None):
        super().__init__(device, seed)
        self.hidden_units = [int(u) for u in hidden_units]
        acts = [activation] * len(self.hidden_units)
        if output_activation and acts:
            acts[-1] = output_activation
        for a in acts:
            if a not in _ACTS:
                raise ValueError(f"unsupported activation {a!r}")
        self.activation, self.output_activation, self.use_bn = activation, output_activation, bool(use_bn)
        self.l2_reg, self.dropout_rate = l2_reg, dropout_rate
        self.layers = nn.ModuleList([Dense(u, activation=a, device=device, seed=_subseed(self._gen))
                                     for u, a in zip(self.hidden_units, acts)])
        self.bn_layers = nn.ModuleList([BatchNormalization(device=device) for _ in self.hidden_units]) \
            if self.use_bn else None
        if input_dim is not None:
            self.build(input_dim)

    @property
    def built(self):
        return not self.layers or self.layers[0].kernel is not None

    def build(self, n):
        for i, l in enumerate(self.layers):
            l.build(n)
            with torch.no_grad():
                l.kernel.copy_(_glorot_normal(n, l.units, self._gen, self._dev))
            if self.use_bn:
                self.bn_layers[i].build(l.units)
            n = l.units

    def keras_weights(self):
        if not self.built:
            raise RuntimeError("DNN: not built (call build(input_dim) or run a forward first)")
        out = {}
        for i, l in enumerate(self.layers):
            out[f"kernel{i}"], out[f"bias{i}"] = l.kernel, l.bias
            if l.alpha is not None:
                out[f"alpha{i}"] = l.alpha
            if l.dice is not None:
                out.update({f"dice{i}/{k}": v for k, v in l.dice.keras_weights().items()})
            if self.use_bn:
                out.update({f"bn{i}/{k}": v for k, v in self.bn_layers[i].keras_weights().items()})
        return out

    def set_keras_weights(self, weights, strict=True):
        own = self.keras_weights()
        if strict and set(own) != set(weights):
            raise KeyError(f"DNN: expected weights {sorted(own)}, got {sorted(weights)}")
        with torch.no_grad():
            for name, p in own.items():
                if name in weights:
                    p.copy_(torch.as_tensor(weights[name], dtype=torch.float32).reshape(p.shape))
        self._weights_changed()

    def forward(self, inputs):
        x = inputs if (torch.is_tensor(inputs) and inputs.is_cuda and inputs.dtype == torch.float32) \
            else _to_device_f32(inputs, self._dev)
        if not self.built:
            self.build(x.shape[-1])
        lead = x.shape[:-1]
        x = x.reshape(-1, x.shape[-1])
        for i, l in enumerate(self.layers):
            M, K = x.shape
            if not self.use_bn:
                x = l(x)  # Dense: rs_dense_fwd with the activation (Dice after it)
                continue
            y = torch.empty(M, l.units, dtype=torch.float32, device=self._dev)
            call("rs_dense_fwd", ptr(x), x.stride(0), ptr(l.kernel), ptr(l.bias), None, 0, ptr(y), y.stride(0), M, K,
                 l.units, _stream())
            inv, shift = self.bn_layers[i].affine()
            act = 0 if l.activation == "dice" else _lib.ACT[l.activation]
            call("rs_affine_act", ptr(y), y.stride(0), ptr(inv), ptr(shift), ptr(l.alpha), act, ptr(y), y.stride(0), M,
                 l.units, _stream())
            x = l.dice(y, out=y) if l.activation == "dice" else y
        return x.reshape(*lead, x.shape[-1])


class LocalActivationUnit(KerasModule):
    """LocalActivationUnit(hidden_units=(64, 32), activation='sigmoid') —
    layer/core.py:55-108: [q, k, q - k, q * k] through DNN(hidden_units,
    activation), then ``kernel`` [last, 1] (glorot-normal) and ``bias`` [1]:
    ``forward([query[B, 1, D], keys[B, T, D]])`` returns [B, T, 1].  This is the
    composed form (rs_dense_fwd per layer); DIEN's fused launch takes its
    weights (dien.hip)."""

    def __init__(self, hidden_units=(64, 32), activation="sigmoid", l2_reg=0, dropout_rate=0, use_bn=False,
                 device=None, seed=None, input_dim=None):
        super().__init__(device, seed)
        self.hidden_units, self.activation = [int(u) for u in hidden_units], activation
        self.dnn = DNN(self.hidden_units, activation, l2_reg, dropout_rate, use_bn, device=device,
                       seed=_subseed(self._gen))
        self.kernel = self.bias = None
        if input_dim is not None:
            self.build(input_dim)

    @property
    def built(self):
        return self.kernel is not None

    def build(self, D):
        D = int(D)
        self.embedding_size = D
        self.dnn.build(4 * D)
        size = 4 * D if not self.hidden_units else self.hidden_units[-1]
        self.kernel = nn.Parameter(_glorot_normal(size, 1, self._gen, self._dev), requires_grad=False)
        self.bias = nn.Parameter(torch.zeros(1, device=self._dev), requires_grad=False)

    def keras_weights(self):
        if not self.built:
            raise RuntimeError("LocalActivationUnit: not built (call build(D) or run a forward first)")
        out = {"kernel": self.kernel, "bias": self.bias}
        out.update({f"dnn/{k}": v for k, v in self.dnn.keras_weights().items()})
        return out

    def set_keras_weights(self, weights, strict=True):
        own = self.keras_weights()
        if strict and set(own) != set(weights):
            raise KeyError(f"LocalActivationUnit: expected weights {sorted(own)}, got {sorted(weights)}")
        with torch.no_grad():
            for name, p in own.items():
                if name in weights:
                    p.copy_(torch.as_tensor(weights[name], dtype=torch.float32).reshape(p.shape))
        self._weights_changed()

    def forward(self, inputs):
        query, keys = inputs
        keys = _seq_input(keys, self._dev, "LocalActivationUnit")
        B, T, D = keys.shape
        q = query if (torch.is_tensor(query) and query.is_cuda) else _to_device_f32(query, self._dev)
        q = q.reshape(B, 1, D).to(torch.float32)
        if not self.built:
            self.build(D)
        if D != self.embedding_size:
            raise ValueError(f"LocalActivationUnit built for width {self.embedding_size}, got {D}")
        qq = q.expand(B, T, D)
        e = torch.cat([qq, keys, qq - keys, qq * keys], dim=-1).reshape(B * T, 4 * D)
        y = self.dnn(e)
        s = torch.empty(B * T, 1, dtype=torch.float32, device=self._dev)
        if B * T:
            call("rs_dense_fwd", ptr(y), y.stride(0), ptr(self.kernel), ptr(self.bias), None, 0, ptr(s), 1, B * T,
                 y.shape[1], 1, _stream())
        return s.reshape(B, T, 1)


class AttentionSequencePoolingLayer(KerasModule):
    """AttentionSequencePoolingLayer(att_hidden_units=(80, 40),
    att_activation='sigmoid', weight_normalization=False, return_score=False)
    — layer/sequence.py:205-273: ``forward([query[B, 1, D], keys[B, T, D],
    keys_length[B, 1]])``: the LocalActivationUnit's scores, positions t >=
    length set to -2**32 + 1 and a softmax over T (weight_normalization) or
    set to 0 (none); returns the scores [B, 1, T] with return_score, else the
    pooled keys scores @ keys [B, 1, D].  (The reference subscripts the method
    ``as_list`` at :248; built as ``as_list()[1]``.)"""

    def __init__(self, att_hidden_units=(80, 40), att_activation="sigmoid", weight_normalization=False,
                 return_score=False, device=None, seed=None, input_dim=None):
        super().__init__(device, seed)
        self.att_hidden_units = [int(u) for u in att_hidden_units]
        self.att_activation = att_activation
        self.weight_normalization, self.return_score = bool(weight_normalization), bool(return_score)
        self.local_att = LocalActivationUnit(self.att_hidden_units, att_activation, device=device,
                                             seed=_subseed(self._gen), input_dim=input_dim)

    def keras_weights(self):
        return {f"local_att/{k}": v for k, v in self.local_att.keras_weights().items()}

    def set_keras_weights(self, weights, strict=True):
        self.local_att.set_keras_weights({k.split("/", 1)[1]: v for k, v in weights.items()
                                          if k.startswith("local_att/")}, strict)

    def forward(self, inputs):
        query, keys, keys_length = inputs
        keys = _seq_input(keys, self._dev, "AttentionSequencePoolingLayer")
        B, T, _ = keys.shape
        s = self.local_att([query, keys]).reshape(B, T)
        L = _lengths(keys_length, self._dev, B)
        valid = torch.arange(T, device=self._dev).unsqueeze(0) < L.unsqueeze(1)
        if self.weight_normalization:
            s = torch.softmax(torch.where(valid, s, torch.full_like(s, float(-2 ** 32 + 1))), dim=-1)
        else:
            s = torch.where(valid, s, torch.zeros_like(s))
        s = s.unsqueeze(1)
        return s if self.return_score else torch.matmul(s, keys)


class InterestEvolution(KerasModule):
    """interest_evolution(...) of model/dien.py:54-80 as a module: ``gru1`` =
    GRU(D, return_sequences=True), ``attention`` = AttentionSequencePoolingLayer(
    att_hidden_units, att_activation, weight_normalization, return_score=True)
    and ``gru2`` = AUGRU(D), on keys [B, T, D], a query [B, D] and lengths [B].

    ``forward(keys, query, seq_length)`` returns hist [B, D].  It is ONE
    rs_dien_evolution_fwd launch (dien.hip: H1 and the scores stay in LDS) when
    ``fused_ok(T)``; otherwise ``forward_unfused``: rs_gru_fwd, the attention
    layer's composed scores, rs_augru_fwd.  ``forward_ids`` takes the behaviour
    features' ids and tables instead of gathered rows (rs_dien_evolution_ids_fwd:
    the keys are never written to HBM).  ``out`` (a [B, >= D] view with unit
    column stride) receives hist in place; ``want_h1`` / ``want_scores`` also
    return H1 [B, T, D] / the scores [B, T]."""

    def __init__(self, embedding_size, att_hidden_units=(64, 16), att_activation="sigmoid",
                 att_weight_normalization=False, gru_type="AUGRU", augru_update="reference", device=None, seed=None):
        super().__init__(device, seed)
        D = int(embedding_size)
        if augru_update not in _DIEN_UPDATES:
            raise ValueError(f"augru_update must be 'reference' or 'paper', got {augru_update!r}")
        self.embedding_size, self.augru_update = D, augru_update
        self.gru1 = GRU(D, return_sequences=True, device=device, seed=_subseed(self._gen), input_dim=D)
        self.attention = AttentionSequencePoolingLayer(att_hidden_units, att_activation, att_weight_normalization,
                                                       return_score=True, device=device, seed=_subseed(self._gen),
                                                       input_dim=D)
        self.gru2 = AUGRU(D, gru_type=gru_type, augru_update=augru_update, device=device, seed=_subseed(self._gen),
                          input_dim=D)

    def keras_weights(self):
        out = {f"gru1/{k}": v for k, v in self.gru1.keras_weights().items()}
        out.update({f"attention_sequence_pooling_layer/{k}": v for k, v in self.attention.keras_weights().items()})
        out.update({f"gru2/{k}": v for k, v in self.gru2.keras_weights().items()})
        return out

    def set_keras_weights(self, weights, strict=True):
        own = self.keras_weights()
        if strict and set(own) != set(weights):
            raise KeyError(f"InterestEvolution: expected weights {sorted(own)}, got {sorted(weights)}")
        with torch.no_grad():
            for name, p in own.items():
                if name in weights:
                    p.copy_(torch.as_tensor(weights[name], dtype=torch.float32).reshape(p.shape))
        self._weights_changed()

    def _hidden(self):
        return ints(self.attention.att_hidden_units)

    def fused_ok(self, T):
        a = self.attention
        act = _DIEN_ACTS.get(a.att_activation)
        return bool(act is not None and not a.local_att.dnn.use_bn and _lib.lib().rs_dien_evolution_ok(
            int(T), self.embedding_size, len(a.att_hidden_units), self._hidden(), act))

    def prepared(self):
        """The weights packed for the one-launch form (rs_dien_prepare), cached until one changes."""
        def build():
            a, la = self.attention, self.attention.local_att
            n, D = len(a.att_hidden_units), self.embedding_size
            prep = sized("rs_dien_prepared_size", D, n, self._hidden(), device=self._dev)
            ls = list(la.dnn.layers)
            dice = a.att_activation == "dice"
            call("rs_dien_prepare", D, ptr(self.gru1.kernel), ptr(self.gru1.recurrent_kernel), ptr(self.gru1.bias),
                 ptr(self.gru2.cell.kernel), ptr(self.gru2.cell.recurrent_kernel), n, self._hidden(),
                 _DIEN_ACTS[a.att_activation], ptrs([l.kernel for l in ls]), ptrs([l.bias for l in ls]),
                 ptrs([l.dice.moving_mean for l in ls]) if dice else None,
                 ptrs([l.dice.moving_variance for l in ls]) if dice else None,
                 ptrs([l.dice.alphas for l in ls]) if dice else None, ptr(la.kernel), ptr(la.bias), ptr(prep),
                 _stream())
            return prep
        return self._packed("dien", list(self.keras_weights().values()), build)

    def _outputs(self, B, T, out, want_h1, want_scores):
        D = self.embedding_size
        if out is None:
            out = torch.empty(B, D, dtype=torch.float32, device=self._dev)
        if out.dim() != 2 or out.shape[0] != B or out.shape[1] < D or (B and out.stride(1) != 1):
            raise ValueError("InterestEvolution: out must be a [batch, >= D] view with unit column stride")
        h1 = torch.empty(B, T, D, dtype=torch.float32, device=self._dev) if want_h1 else None
        sc = torch.empty(B, T, dtype=torch.float32, device=self._dev) if want_scores else None
        return out, h1, sc

    def _tail_args(self, T):
        a = self.attention
        return (T, self.embedding_size, len(a.att_hidden_units), self._hidden(), _DIEN_ACTS[a.att_activation],
                1 if a.weight_normalization else 0, _DIEN_UPDATES[self.augru_update], ptr(self.prepared()))

    @staticmethod
    def _ret(out, h1, sc, want_h1, want_scores):
        if not (want_h1 or want_scores):
            return out
        return (out,) + ((h1,) if want_h1 else ()) + ((sc,) if want_scores else ())

    def forward_fused(self, keys, query, seq_length, out=None, want_h1=False, want_scores=False):
        keys = _seq_input(keys, self._dev, "InterestEvolution")
        B, T, D = keys.shape
        if D != self.embedding_size:
            raise ValueError(f"InterestEvolution built for width {self.embedding_size}, got {D}")
        q = query if (torch.is_tensor(query) and query.is_cuda and query.dtype == torch.float32) \
            else _to_device_f32(query, self._dev)
        q = q.reshape(B, D)
        q = q if (not B or q.stride(1) == 1) else q.contiguous()
        L = _lengths(seq_length, self._dev, B)
        out, h1, sc = self._outputs(B, T, out, want_h1, want_scores)
        call("rs_dien_evolution_fwd", ptr(keys), keys.stride(0), keys.stride(1), ptr(q), q.stride(0), ptr(L),
             _lib.id_kind(L), *self._tail_args(T), ptr(h1), ptr(sc), ptr(out), out.stride(0), B, _stream())
        return self._ret(out[:, :D], h1, sc, want_h1, want_scores)

    def forward_ids(self, hist_ids, cand_ids, tables, seq_length, out=None, want_h1=False, want_scores=False,
                    check_ids=True, err=None):
        """hist_ids[f] [B, T], cand_ids[f] [B] and tables[f] [vocab_f, width_f]
        per behaviour feature (1..4, widths adding up to D).  err: the caller's
        device error flag (its own check follows), else one is made here."""
        n = len(tables)
        hs = [_ids_tensor(h, self._dev) for h in hist_ids]
        cs = [_ids_tensor(c, self._dev).reshape(-1).to(h.dtype).contiguous() for c, h in zip(cand_ids, hs)]
        hs = [h if h.stride(1) == 1 else h.contiguous() for h in hs]
        B, T = hs[0].shape
        L = _lengths(seq_length, self._dev, B)
        out, h1, sc = self._outputs(B, T, out, want_h1, want_scores)
        err = err if err is not None else _ErrFlag(self._dev)
        la = lambda v: (C.c_int64 * n)(*v)
        call("rs_dien_evolution_ids_fwd", n, ints([t.shape[1] for t in tables]), ints([_lib.id_kind(h) for h in hs]),
             ptrs(hs), la([h.stride(0) for h in hs]), ptrs(cs), la([1] * n), ptrs(tables),
             la([t.shape[0] for t in tables]),
             ptr(L), _lib.id_kind(L), *self._tail_args(T), ptr(h1), ptr(sc), ptr(out), out.stride(0), B, ptr(err.t),
             _stream())
        if check_ids:
            err.check("InterestEvolution")
        return self._ret(out[:, :self.embedding_size], h1, sc, want_h1, want_scores)

    def forward_unfused(self, keys, query, seq_length, out=None, want_h1=False, want_scores=False):
        keys = _seq_input(keys, self._dev, "InterestEvolution")
        B, T, D = keys.shape
        h1 = self.gru1(keys)
        sc = self.attention([query, h1, seq_length]).reshape(B, T)
        hist = self.gru2(h1, sc)
        if out is not None:
            out[:, :D] = hist
            hist = out[:, :D]
        return self._ret(hist, h1, sc, want_h1, want_scores)

    def train_forward(self, keys, query, seq_length):
        """The forward of a training step: (hist [B, D], H1 [B, T, D], ctx).
        Always the composed form — rs_gru_train_fwd; the attention unit at M =
        B T rows (rs_din_att_concat for [q, k, q - k, q k], rs_dense_fwd per
        layer, then rs_dice_train_fwd or relu / sigmoid, the score Dense, mask
        and softmax); rs_augru_train_fwd.  'dice' runs in training mode, as
        Dice.call(training=True) does: the batch's statistics over all B T
        rows, padded positions included, moving averages moved with momentum
        0.99 — which the one-launch kernel cannot provide.  relu / sigmoid, the
        mask and the softmax are torch elementwise ops.  ctx is what
        ``train_backward`` reads."""
        a, la = self.attention, self.attention.local_att
        if la.dnn.use_bn or any(l.activation not in ("relu", "sigmoid", "dice") for l in la.dnn.layers):
            raise NotImplementedError("InterestEvolution.train_forward: att_activation 'relu', 'sigmoid' or 'dice' only")
        st = _stream()
        keys = _seq_input(keys, self._dev, "InterestEvolution").contiguous()
        B, T, D = keys.shape
        if D != self.embedding_size:
            raise ValueError(f"InterestEvolution built for width {self.embedding_size}, got {D}")
        q = query if (torch.is_tensor(query) and query.is_cuda and query.dtype == torch.float32) \
            else _to_device_f32(query, self._dev)
        q = q.reshape(B, D).contiguous()
        L = _lengths(seq_length, self._dev, B)
        M, layers = B * T, list(la.dnn.layers)
        shapes = [(l.kernel.shape[0], l.kernel.shape[1], M) for l in layers] + [(la.kernel.shape[0], 1, M)]
        dt = _train_ops.DenseTrain(_train_ops.gemm_ws(self, _train_ops.dense_train_need(shapes)), st, self._dev)
        H1, sv1 = _train_ops.gru_train_forward(self.gru1, keys, st)
        e0 = dt.emp(M, 4 * D)
        call("rs_din_att_concat", ptr(q), ptr(H1), B, T, D, ptr(e0), st)
        a_in, a_pre, a_saved = [e0], [], []
        for l in layers:
            z = dt.dense(a_in[-1], l, M)
            saved, y = dt.act_fwd(l, z, M)
            a_pre.append(z), a_saved.append(saved), a_in.append(y)
        raw = dt.dense(a_in[-1], la, M).reshape(B, T)
        valid = torch.arange(T, device=self._dev).unsqueeze(0) < L.unsqueeze(1)
        if a.weight_normalization:
            scores = torch.softmax(torch.where(valid, raw, torch.full_like(raw, float(-2 ** 32 + 1))), dim=-1)
        else:
            scores = torch.where(valid, raw, torch.zeros_like(raw))
        hist, sv2 = _train_ops.augru_train_forward(self.gru2, H1, scores, st)
        ctx = dict(keys=keys, q=q, L=L, H1=H1, sv1=sv1, sv2=sv2, scores=scores, a_in=a_in, a_pre=a_pre,
                   a_saved=a_saved, dt=dt)
        return hist, H1, ctx

    def train_backward(self, ctx, dhist, dh1=None):
        """The backward of ``train_forward`` from dhist = dL/d(hist) [B, D] and,
        optionally, dh1 = a gradient that reaches H1 from elsewhere (DIEN's
        auxiliary loss) [B, T, D]: rs_augru_bwd (the chain and the scores'
        gradient through the mask), the attention unit reversed (split-K
        rs_gemm / rs_col_sum_split, rs_dice_train_bwd) into
        rs_din_att_concat_bwd, which adds into dH1 and dq, then rs_gru_bwd.
        Returns (dkeys [B, T, D], dq [B, D], [(weight, gradient, l2)]) for every
        weight of ``keras_weights()`` that trains; nothing is updated here."""
        a, la = self.attention, self.attention.local_att
        dt, st, H1, q = ctx["dt"], ctx["dt"].st, ctx["H1"], ctx["q"]
        B, T, D = H1.shape
        M, layers = B * T, list(la.dnn.layers)
        first = len(dt.updates)
        dH1, ds, _, dW2, dU2 = _train_ops.augru_backward(self.gru2, H1, ctx["scores"], ctx["L"], a.weight_normalization,
                                                         ctx["sv2"], dhist, st)
        c2 = self.gru2.cell
        dt.updates.extend([(c2.kernel, dW2, 0.0), (c2.recurrent_kernel, dU2, 0.0)])
        a_in, a_pre, a_saved = ctx["a_in"], ctx["a_pre"], ctx["a_saved"]
        d_in = dt.dense_bwd(la, a_in[-1], ds.reshape(M, 1))
        for i in reversed(range(len(layers))):
            dz = dt.act_bwd(layers[i], a_pre[i], a_in[i + 1], a_saved[i], d_in, M)
            d_in = dt.dense_bwd(layers[i], a_in[i], dz)
        dq = torch.zeros(B, D, dtype=torch.float32, device=self._dev)
        call("rs_din_att_concat_bwd", ptr(d_in), ptr(q), ptr(H1), B, T, D, ptr(dq), D, ptr(dH1), st)
        if dh1 is not None:
            dH1 += dh1
        g1 = self.gru1
        dkeys, dW1, dU1, db1 = _train_ops.gru_backward(g1, ctx["keys"], ctx["sv1"], dH1, None, st)
        dt.updates.extend([(g1.kernel, dW1, 0.0), (g1.recurrent_kernel, dU1, 0.0), (g1.bias, db1, 0.0)])
        return dkeys, dq, dt.updates[first:]

    def forward(self, keys, query, seq_length, **kw):
        T = torch.as_tensor(keys).shape[1] if not torch.is_tensor(keys) else keys.shape[1]
        return (self.forward_fused if self.fused_ok(T) else self.forward_unfused)(keys, query, seq_length, **kw)


class PredictionLayer(KerasModule):
    """PredictionLayer(task='binary', use_bias=True) — layer/core.py:223-256:
    sigmoid(x + global_bias) for 'binary', x + global_bias for 'regression';
    ``global_bias`` [1] zeros.  Output [B, 1]."""

    def __init__(self, task="binary", use_bias=True, device=None):
        super().__init__(device)
        if task not in ("binary", "multiclass", "regression"):
            raise ValueError("task must be binary,multiclass or regression")
        self.task, self.use_bias = task, bool(use_bias)
        self.global_bias = nn.Parameter(torch.zeros(1, device=self._dev), requires_grad=False) if use_bias else None
        self._one = None

    def forward(self, inputs):
        x = inputs if (torch.is_tensor(inputs) and inputs.is_cuda and inputs.dtype == torch.float32) \
            else _to_device_f32(inputs, self._dev)
        x = x.reshape(-1, 1).contiguous()
        if self._one is None:
            self._one = torch.ones(1, device=self._dev)
            self._zero = torch.zeros(1, device=self._dev)
        out = torch.empty_like(x)
        if x.shape[0]:
            call("rs_affine_act", ptr(x), 1, ptr(self._one), ptr(self.global_bias if self.use_bias else self._zero),
                 None, _lib.ACT["sigmoid"] if self.task == "binary" else 0, ptr(out), 1, x.shape[0], 1, _stream())
        return out


# ------------------------------------------------------------------- DSSM
_COMBINERS = {"sum": 0, "mean": 1, "max": 2}
_SEQ_MAXF, _SEQ_MAXE = 8, 256  # rs_seq_pool_fwd limits (dssm.hip)


def seq_pool_ok(E):
    """Widths rs_seq_pool_fwd takes: 1..64, or a multiple of 4 up to 256."""
    return E >= 1 and (E <= 64 or (E % 4 == 0 and E <= _SEQ_MAXE))


def seq_pool_arrays(feats):
    """The thirteen per-feature host arrays of rs_seq_pool_fwd (and of the
    sequence pieces of rs_dssm_tower_fwd) for feats = [(E, column, T, combiner,
    source, table or None, lengths or None, mask or None)]: source = ids [B, T]
    with a table, embedded values [B, T, E] without."""
    n = len(feats)
    cl = lambda v: (C.c_int64 * n)(*v)
    kinds = [-1 if f[5] is None else _lib.id_kind(f[4]) for f in feats]
    return (ints([f[0] for f in feats]), ints([f[1] for f in feats]), ints([f[2] for f in feats]),
            ints([_COMBINERS[f[3]] for f in feats]), ints(kinds), ptrs([f[4] for f in feats]),
            cl([f[4].stride(0) for f in feats]), ptrs([f[5] for f in feats]),
            cl([0 if f[5] is None else f[5].shape[0] for f in feats]), ptrs([f[6] for f in feats]),
            ints([0 if f[6] is None else _lib.id_kind(f[6]) for f in feats]), ptrs([f[7] for f in feats]))


def seq_pool(feats, out, B, err):
    """rs_seq_pool_fwd over feats (seq_pool_arrays) into out [B, *], 8 features a launch."""
    for i in range(0, len(feats) if B else 0, _SEQ_MAXF):
        ch = feats[i:i + _SEQ_MAXF]
        call("rs_seq_pool_fwd", len(ch), *seq_pool_arrays(ch), ptr(out), out.stride(0), B, ptr(err.t), _stream())


def l2_normalize(x, out=None):
    """tf.math.l2_normalize(x, axis=-1) of x [M, N]: rs_l2_normalize_fwd."""
    if out is None:
        out = torch.empty(x.shape[0], x.shape[1], dtype=torch.float32, device=x.device)
    call("rs_l2_normalize_fwd", ptr(x), x.stride(0), ptr(out), out.stride(0), x.shape[0], x.shape[1], _stream())
    return out


class SequencePoolingLayer(KerasModule):
    """SequencePoolingLayer(mode='mean', supports_masking=False) —
    layer/sequence.py:20-95: sum / mean / max pooling of a variable-length
    sequence, one rs_seq_pool_fwd launch.  ``forward([seq_value [B, T, E],
    seq_len [B] or [B, 1]])``, or with ``supports_masking=True``
    ``forward(seq_value, mask=[B, T] bool)``; returns [B, 1, E].
    ``forward_ids(ids [B, T], table [vocab, E], lengths=None, out=None)`` pools
    straight from the ids — masked rows are never loaded — and returns [B, E];
    ``lengths=None`` is the reference's mask_zero form (mask = id != 0)."""

    def __init__(self, mode="mean", supports_masking=False, device=None):
        super().__init__(device)
        if mode not in ("sum", "mean", "max"):
            raise ValueError("mode must be sum or mean")
        self.mode, self.supports_masking = mode, bool(supports_masking)

    def _run(self, feat, B, E, out, check_ids, what):
        if not seq_pool_ok(E):
            raise _lib.RSError(f"{what}: width {E} not supported (1..64, or a multiple of 4 up to {_SEQ_MAXE})")
        if out is None:
            out = torch.empty(B, E, dtype=torch.float32, device=self._dev)
        err = _ErrFlag(self._dev)
        seq_pool([(E, 0, feat[0], self.mode) + feat[1:]], out, B, err)
        if check_ids:
            err.check(what)
        return out

    def forward(self, seq_value_len_list, mask=None):
        if self.supports_masking:
            if mask is None:
                raise ValueError("When supports_masking=True,input must support masking")
            x = _seq_input(seq_value_len_list, self._dev, "SequencePoolingLayer").contiguous()
            m = torch.as_tensor(mask).to(self._dev).reshape(x.shape[0], x.shape[1]).ne(0).contiguous()
            L = None
        else:
            x, L = seq_value_len_list
            x = _seq_input(x, self._dev, "SequencePoolingLayer").contiguous()
            L, m = _lengths(L, self._dev, x.shape[0]), None
        B, T, E = x.shape
        return self._run((T, x, None, L, m), B, E, None, False, "SequencePoolingLayer").unsqueeze(1)

    def forward_ids(self, ids, table, lengths=None, out=None, check_ids=True):
        ids = _ids_tensor(ids, self._dev).contiguous()
        if ids.dim() != 2:
            raise ValueError(f"SequencePoolingLayer.forward_ids: ids must be [batch, T], got {tuple(ids.shape)}")
        B, T = ids.shape
        L = None if lengths is None else _lengths(lengths, self._dev, B)
        return self._run((T, ids, table, L, None), B, table.shape[1], out, check_ids,
                         "SequencePoolingLayer.forward_ids")


class InBatchSoftmaxLayer(KerasModule):
    """InBatchSoftmaxLayer(sampler_config, temperature=1.0) —
    layer/activation.py:267-285 with layer/utils.py:206-215:
    ``forward([user_vec [B, E], item_vec [B, E], item_idx [B] or [B, 1]])``
    returns the per-sample loss [B, 1],
        logits = (user / temperature) @ item^T - log Q[item_idx]   (per column)
        loss_i = logsumexp_j logits_ij - logits_ii
    in one rs_inbatch_softmax_fwd launch — the [B, B] logits are never written.
    ``sampler_config``: a NegativeSampler or its ``_asdict()``; log Q is built
    once, as the reference builds it: float32(item_count / sum(item_count))
    (divided in float64), then a float32 log.  A width the kernel refuses
    (rs_inbatch_softmax_ok) runs the same composition in torch ops."""

    def __init__(self, sampler_config, temperature=1.0, device=None):
        super().__init__(device)
        import numpy as np
        cfg = sampler_config._asdict() if hasattr(sampler_config, "_asdict") else dict(sampler_config)
        self.sampler_config, self.temperature = cfg, float(temperature)
        self.item_count = cfg["item_count"]
        if self.item_count is None:
            raise ValueError(" `item_count` must not be `None` when using `inbatch` or `frequency` sampler")
        q = (np.asarray(self.item_count) / np.sum(self.item_count)).astype(np.float32)
        with np.errstate(divide="ignore"):
            self.logq = torch.from_numpy(np.log(q)).to(self._dev)

    def forward(self, inputs_with_item_idx, check_ids=True):
        u, v, idx = inputs_with_item_idx
        u, v = _to_device_f32(u, self._dev), _to_device_f32(v, self._dev)
        idx = torch.as_tensor(idx)
        if idx.dtype not in (torch.int32, torch.int64):
            idx = idx.to(torch.int64)
        idx = idx.to(self._dev).reshape(-1).contiguous()
        B, E = u.shape
        if v.shape != u.shape or idx.numel() != B:
            raise ValueError(f"InBatchSoftmaxLayer: user {tuple(u.shape)}, item {tuple(v.shape)}, "
                             f"{idx.numel()} item indices")
        if not _lib.lib().rs_inbatch_softmax_ok(E):
            z = (u / self.temperature) @ v.t() - self.logq[idx.long()].unsqueeze(0)
            return (torch.logsumexp(z, dim=1) - torch.diagonal(z)).unsqueeze(1)
        loss = torch.empty(B, 1, dtype=torch.float32, device=self._dev)
        err = _ErrFlag(self._dev)
        call("rs_inbatch_softmax_fwd", ptr(u), u.stride(0), ptr(v), v.stride(0), ptr(idx), _lib.id_kind(idx),
             ptr(self.logq), self.logq.numel(), self.temperature, ptr(loss), B, E, ptr(err.t), _stream())
        if check_ids:
            err.check("InBatchSoftmaxLayer")
        return loss
