"""CPU: host-side logic of the Keras-compatible layers/models (construction,
Keras-shaped weights and names, initialiser statistics, error behaviour).
Modules are built on the CPU device; no kernel is launched."""
import numpy as np
import pytest
import torch
from torch import nn

from recommender_system_amd import (DCN, PNN, Attention, CrossLayer, DeepFM, Dense, DNNLayer, EmbedLayer, FMLayer)
from recommender_system_amd.layers import KerasModule
from tests.helpers import criteo_columns

DEV = "cpu"


def test_embed_layer_layout_and_names():
    cols = criteo_columns([5, 7, 3])[1]
    e = EmbedLayer(cols, k=4, device=DEV, seed=0)
    assert e.table.shape == (15, 4) and e.row_offsets == [0, 5, 12]
    assert e.field_table(1).shape == (7, 4)
    w = e.keras_weights()
    assert list(w) == ["embedding_0/embeddings", "embedding_1/embeddings", "embedding_2/embeddings"]
    assert float(e.table.abs().max()) <= 0.05  # Keras Embedding U(-0.05, 0.05)
    new = {k: np.full(v.shape, i, np.float32) for i, (k, v) in enumerate(w.items())}
    e.set_keras_weights(new)
    assert float(e.field_table(2).mean()) == 2.0


def test_embed_layer_default_k_is_8_and_ignores_embed_dim():
    cols = criteo_columns([5, 7], embed_dim=32)[1]
    assert EmbedLayer(cols, device=DEV).k == 8  # layer/core.py:268-271


def test_fm_layer_keras_shapes_and_init():
    fm = FMLayer(10, device=DEV, seed=1, input_dim=429)
    w = fm.keras_weights()
    assert w["w0"].shape == (1,) and w["w1"].shape == (429, 1) and w["v"].shape == (429, 10)
    assert float(w["w0"]) == 0.0
    assert abs(float(w["v"].std()) - 0.05) < 0.005  # random_normal_initializer stddev 0.05


def test_cross_layer_weights():
    c = CrossLayer(3, device=DEV, seed=2, input_dim=20)
    w = c.keras_weights()
    assert sorted(w) == ["b0", "b1", "b2", "w0", "w1", "w2"]
    assert all(v.shape == (20, 1) for v in w.values())


def test_dense_glorot_and_prelu_alpha():
    d = Dense(256, "prelu", device=DEV, seed=3, input_dim=429)
    lim = np.sqrt(6 / (429 + 256))
    assert float(d.kernel.abs().max()) <= lim and d.kernel.shape == (429, 256)
    assert float(d.alpha.abs().sum()) == 0.0 and d.alpha.shape == (256,)


def test_dnn_layer_structure():
    dnn = DNNLayer([256, 128, 64], 1, "relu", device=DEV, seed=4)
    dnn.build(429)
    shapes = [tuple(v.shape) for v in dnn.keras_weights().values()]
    assert shapes == [(429, 256), (256,), (256, 128), (128,), (128, 64), (64,), (64, 1), (1,)]


def test_models_construct_with_reference_signatures():
    cols = criteo_columns(np.full(26, 50))
    m = DeepFM(cols, 10, 1e-4, 1e-4, [256, 128, 64], 1, "relu", embed_dim=16, device=DEV)
    assert m.fm.v.shape == (13 + 26 * 16, 10)
    m2 = DCN(cols, [256, 128, 64], 1, "relu", layer_num=3, device=DEV, embed_dim=16)
    assert m2.output_layer.kernel.shape == (429 + 1, 1)
    m3 = PNN(cols, "inner", [256, 128, 64], 1, device=DEV, embed_dim=16)
    assert m3.width == 26 * 16 + 325


def test_pnn_mode_errors():
    cols = criteo_columns([5] * 4)
    with pytest.raises(ValueError, match="Please choice mode"):
        PNN(cols, "bogus", [8], 1, device=DEV)
    m = PNN(cols, "both", [8], 1, device=DEV, embed_dim=4)  # outer/both are built (OuterProductLayer)
    assert m.width == 4 * 4 + 2 * 6 and tuple(m.outer_product_layer.W.shape) == (4, 6, 4)
    with pytest.raises(NotImplementedError):
        PNN(cols, "inner", [8], 1, use_fgcnn=True, device=DEV)


def test_attention_prelu_alpha_shape_is_T_by_h():
    att = Attention((80, 40), "prelu", device=DEV, seed=5)
    att.build(100, 8)
    w = att.keras_weights()
    assert w["dense_0/kernel"].shape == (32, 80) and w["dense_0/prelu/alpha"].shape == (100, 80)
    assert w["dense_1/prelu/alpha"].shape == (100, 40) and w["out/kernel"].shape == (40, 1)
    with pytest.raises(ValueError):
        Attention((80, 40), "sigmoid", device=DEV)


def test_attention_dice_has_no_dense():
    att = Attention((80, 40), "dice", device=DEV)
    att.build(10, 8)
    w = att.keras_weights()
    assert not any(k.startswith("dense_") for k in w)
    assert w["dice_0/dice_alpha"].shape == (32,) and w["out/kernel"].shape == (32, 1)


def test_scratch_is_one_grow_only_buffer_per_owner_and_name():
    """_train_ops.scratch: the first call allocates, a smaller request returns
    the same tensor object, a larger one a larger tensor, and two names on
    one owner are independent."""
    from recommender_system_amd._train_ops import scratch
    owner = Dense(3, device=DEV, seed=0)  # any module with a device; its buffers live in owner.__dict__
    a = scratch(owner, "_emb_ws", 100)
    assert a.dtype == torch.uint8 and a.numel() == 100 and a.device.type == "cpu"
    assert owner.__dict__["_emb_ws"] is a
    assert scratch(owner, "_emb_ws", 40) is a and scratch(owner, "_emb_ws", 100) is a
    b = scratch(owner, "_emb_ws", 101)
    assert b is not a and b.numel() == 101 and owner.__dict__["_emb_ws"] is b
    c = scratch(owner, "_gemm_wsbuf", 7)
    assert c.numel() == 7 and scratch(owner, "_emb_ws", 1) is b and scratch(owner, "_gemm_wsbuf", 7) is c


class _Packs(KerasModule):
    """Two CPU parameters, a child KerasModule, and a ``build`` that counts."""

    def __init__(self, child=True):
        super().__init__(DEV, 0)
        self.a = nn.Parameter(torch.zeros(3), requires_grad=False)
        self.b = nn.Parameter(torch.ones(2), requires_grad=False)
        self.child = _Packs(child=False) if child else None
        self.built = []

    def build(self):
        self.built.append(object())
        return self.built[-1]

    def image(self, slot="img", extra=()):
        return self._packed(slot, (self.a, self.b), self.build, extra)


def test_packed_cache_rebuilds_exactly_when_a_weight_or_extra_changes():
    """KerasModule._packed: one entry per slot, keyed on every parameter's
    (version, storage) and on ``extra``; ``_weights_changed`` drops the
    module's and its children's entries; nothing of it is module state."""
    m = _Packs()
    v = m.image()
    assert v is m.built[0] and len(m.built) == 1  # the value is what build returned
    assert m.image() is v and len(m.built) == 1   # a second lookup does not rebuild
    with torch.no_grad():
        m.a.add_(1)                               # an in-place update bumps the version
    v2 = m.image()
    assert v2 is m.built[1] and v2 is not v and m.image() is v2 and len(m.built) == 2
    ver = m.b._version
    m.b.data = torch.ones(2)                      # new storage under the same parameter
    assert m.b._version == ver
    v3 = m.image()
    assert v3 is m.built[2] and m.image() is v3 and len(m.built) == 3
    # extra: one entry per slot, so going back to the first value rebuilds again
    x = m.image(extra=(1, 2))
    assert len(m.built) == 4 and m.image(extra=(1, 2)) is x and len(m.built) == 4
    y = m.image(extra=(3, 4))
    assert len(m.built) == 5 and y is not x
    assert m.image(extra=(1, 2)) is m.built[5] and len(m.built) == 6
    # two slots are independent
    o = m.image("other")
    assert len(m.built) == 7 and m.image("other") is o and m.image(extra=(1, 2)) is m.built[5]
    with torch.no_grad():
        m.a.add_(1)
    assert m.image("other") is m.built[7] and len(m.built) == 8
    assert m.image(extra=(1, 2)) is m.built[8] and len(m.built) == 9
    # the raw-pointer hook: the parent's and the child's next lookups rebuild, once each
    c = m.child.image()
    assert m.child.image() is c and len(m.child.built) == 1
    m._weights_changed()
    assert m.image(extra=(1, 2)) is m.built[9] and m.image("other") is m.built[10] and len(m.built) == 11
    assert m.child.image() is m.child.built[1] and m.child.image() is m.child.built[1] and len(m.child.built) == 2
    # not module state
    assert sorted(m.state_dict()) == ["a", "b", "child.a", "child.b"]
    assert sorted(n for n, _ in m.named_parameters()) == ["a", "b", "child.a", "child.b"]
    assert not m._buffers and list(m._modules) == ["child"]


def test_dropout_take_rounds_to_counters_and_rel_accumulates():
    """_Dropout.take: every range starts at a multiple of 4 elements (one
    Philox counter gives 4) and ``rel`` is the running total; ``offset`` adds
    the device counter."""
    from recommender_system_amd import models as M
    rng = M._Dropout(2 ** 64 + 5, device=DEV)
    assert rng.seed == 5 and rng.rel == 0 and int(rng.base) == 0
    assert [rng.take(n) for n in (1, 4, 5, 0, 33 * 32)] == [0, 4, 8, 16, 16]
    assert rng.rel == 16 + 33 * 32 and rng.offset == rng.rel
    rng.base += 40  # what end_step's rs_dropout_advance does on the device
    assert rng.take(3) == 16 + 33 * 32 and rng.offset == 40 + 16 + 33 * 32 + 4
