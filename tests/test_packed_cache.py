"""GPU: no packed weight image survives a training step.

Every model with a packed forward and a ``train_step`` runs forward, forward,
step, forward, step, step, forward at a batch of 17 (one full 16-row tile and
a partial one) with ``_lib.call`` recorded: a repeated forward packs nothing,
the forward after a step packs again exactly what the first one packed, and
its output is bit for bit that of a freshly constructed model given the
trained weights.  The training steps write weights through raw pointers, so
only ``KerasModule._weights_changed`` stands between them and a stale image."""
from collections import Counter

import numpy as np
import pytest
import torch

from oracle import ctr_oracle as O
from tests.helpers import criteo_columns

B = 17
SCRIPT = ("forward", "forward", "step", "forward", "step", "step", "forward")


class Case:
    """make(): a built model; forward(m) / step(m); ok(m): the packed path is
    taken; fused_bwd: the step packs a backward image of its own."""

    def __init__(self, make, forward, step, ok, fused_bwd=False):
        self.make, self.forward, self.step, self.ok, self.fused_bwd = make, forward, step, ok, fused_bwd


def _criteo(seed, n_dense=13, n_fields=26):
    rng = np.random.default_rng(seed)
    vocab = rng.integers(2, 9, n_fields)
    dense = rng.random((B, n_dense)).astype(np.float32)
    ids = np.stack([rng.integers(0, v, B) for v in vocab], 1).astype(np.int32)
    return vocab, dense, ids, rng.integers(0, 2, B).astype(np.float32)


def _criteo_case(make, ok, seed, **step_kw):
    vocab, dense, ids, t = _criteo(seed)
    return Case(lambda: make(vocab), lambda m: m((dense, ids)), lambda m: m.train_step((dense, ids), t, lr=0.1, **step_kw),
                ok)


def case_fm(gpu):
    import recommender_system_amd as rs
    vocab, dense, ids, t = _criteo(1)
    offs = np.concatenate([[0], np.cumsum(vocab)[:-1]])
    x = torch.as_tensor(O.onehot_matrix(dense, ids, vocab), dtype=torch.float32, device=gpu)

    def make():
        m = rs.FM(8, 1e-3, 2e-3, seed=3)
        m.fm.build(13 + int(vocab.sum()))
        return m
    return Case(make, lambda m: m(x), lambda m: m.train_step(dense, ids, t, offs, vocab, lr=0.1), lambda m: True)


def case_deepfm(gpu):
    import recommender_system_amd as rs
    return _criteo_case(lambda v: rs.DeepFM(criteo_columns(v, embed_dim=8), 10, 1e-3, 2e-3, [32, 16], 1, "relu",
                                            embed_dim=8, seed=2), lambda m: m.fused_ok(), 2)


def case_dcn(gpu):
    import recommender_system_amd as rs
    return _criteo_case(lambda v: rs.DCN(criteo_columns(v, embed_dim=8), [32, 16], 1, "relu", layer_num=2, embed_dim=8,
                                         seed=3), lambda m: m.fused_ok(), 3)


def case_pnn(gpu):
    import recommender_system_amd as rs
    return _criteo_case(lambda v: rs.PNN(criteo_columns(v, embed_dim=4), "both", [8], 1, "relu", embed_dim=4, seed=4),
                        lambda m: m.dnn_layer.tower_ok(), 4)


def case_din(gpu):
    import recommender_system_amd as rs
    from tests.test_din import din_columns, din_inputs
    rng = np.random.default_rng(5)
    cols, behaviour = din_columns(1, 8, item_vocab=50, cate_vocab=9, user_vocab=17)
    T = 12
    inputs = din_inputs(rng, cols, behaviour, B, T)
    t = rng.integers(0, 2, B).astype(np.float32)

    def make():
        # DIN builds its layers on the first call (and that call runs them one by one): build them here
        m = rs.DIN(cols, behaviour, att_hidden_units=(16, 8), dnn_hidden_units=(32, 16), seed=4)
        K = sum(l.k for l in m.embed_seq_layers)
        n = 2 * K + sum(l.k for l in m.embed_sparse_layers) + m.dense_num
        m.att_layer.build(T, K)
        m.bn_layer.build(n)
        for layer in list(m.dense_layer) + [m.out_layer]:
            layer.build(n)
            n = layer.units
        return m
    return Case(make, lambda m: m(inputs), lambda m: m.train_step(inputs, t, lr=0.1),
                lambda m: m.tower_ok() and m.att_layer.ids_ok(8))


def case_nfm(gpu):
    import recommender_system_amd as rs
    return _criteo_case(lambda v: rs.NFM(criteo_columns(v, embed_dim=4), [8], 1, embed_dim=4, seed=2),
                        lambda m: m.tower_ok(), 6)


def case_deepcrossing(gpu):
    import recommender_system_amd as rs
    c = _criteo_case(lambda v: rs.DeepCrossing(criteo_columns(v, embed_dim=4), 32, [8], 2, embed_dim=4, seed=0),
                     lambda m: m.fused_ok(), 7, fused=True)
    c.fused_bwd = True
    return c


def case_widedeep(gpu):
    from tests.test_widedeep_train import ND, F, _build, onehot
    vocab, dense, ids, t = _criteo(8, ND, F)
    widths = np.array(vocab, np.int64)
    offsets = np.concatenate([[0], np.cumsum(widths)[:-1]])
    X = np.concatenate([dense, ids, dense, onehot(ids, offsets, widths)], axis=1).astype(np.float32)
    c = dict(vocabs=[int(v) for v in vocab], hidden=[16, 8])
    return Case(lambda: _build(c, gpu), lambda m: m(X), lambda m: m.train_step(X, t, lr=0.1, dropout=False),
                lambda m: m.deep.tower_ok())


def case_mmoe(gpu):
    from tests.test_mmoe_train import _model, make_case
    c = make_case("toy-B19")
    x, labels = c.x[:B], c.labels[:, :B]
    return Case(lambda: _model(gpu, c), lambda m: m(x), lambda m: m.train_step(x, labels, lr=0.01, fused=True),
                lambda m: m.fused_ok() and m.train_fused_ok(), fused_bwd=True)


def case_dien(gpu):
    from tests.test_dien_train import make_model
    _, x, y = make_model("wide", "defaults", "cpu")
    x, y = {k: v[:B] for k, v in x.items()}, y[:B]
    return Case(lambda: make_model("wide", "defaults", gpu)[0], lambda m: m(x), lambda m: m.train_step(x, y, lr=0.1),
                lambda m: m.evolution.fused_ok(m.maxlen) and m.tower_fused_ok())


def case_dssm(gpu):
    from tests.test_dssm import gpu_model, model_case
    x = model_case("demo", B)[2]
    return Case(lambda: gpu_model("demo", gpu, B)[0], lambda m: m(x), lambda m: m.train_step(x),
                lambda m: m.user_tower.fused_ok() and m.item_tower.fused_ok())


CASES = {"FM": case_fm, "DeepFM": case_deepfm, "DCN": case_dcn, "PNN-both": case_pnn, "DIN": case_din, "NFM": case_nfm,
         "DeepCrossing": case_deepcrossing, "WideDeep": case_widedeep, "MMOE": case_mmoe, "DIEN": case_dien,
         "DSSM": case_dssm}


def record_calls(setattr_):
    """Wrap ``_lib.call`` (and the name every module of the package bound at
    import) so that each entry name lands in the returned list."""
    import sys

    import recommender_system_amd as rs
    from recommender_system_amd import _lib
    real, names = _lib.call, []

    def call(name, *args):
        names.append(name)
        return real(name, *args)
    for modname, mod in list(sys.modules.items()):
        if modname.startswith(rs.__name__ + ".") and getattr(mod, "call", None) is real:
            setattr_(mod, "call", call)
    return names


def run_script(c, names):
    """SCRIPT on a new model: (model, per act its entry names, its forwards'
    outputs, its weights after each step)."""
    m = c.make()
    trace, outs, weights = [], [], []
    for act in SCRIPT:
        del names[:]
        if act == "forward":
            outs.append(c.forward(m))
        else:
            c.step(m)
            weights.append({k: v.detach().clone() for k, v in m.keras_weights().items()})
        trace.append(list(names))
    return m, trace, outs, weights


def _tensors(y):
    return [y] if torch.is_tensor(y) else [t for v in y for t in _tensors(v)]


def _packs(names, suffix=""):
    return Counter(n for n in names if "_prepare" in n and n.endswith(suffix))


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_no_packed_image_survives_a_train_step(gpu, monkeypatch, name):
    c = CASES[name](gpu)
    names = record_calls(monkeypatch.setattr)
    m, trace, outs, weights = run_script(c, names)
    assert c.ok(m), "the case must take the packed path"
    first = _packs(trace[0])
    assert first, "the first forward packs its weights"
    assert not _packs(trace[1]), f"a repeated forward packed again: {_packs(trace[1])}"
    assert _packs(trace[3]) == first and _packs(trace[6]) == first, (first, _packs(trace[3]), _packs(trace[6]))
    if c.fused_bwd:  # the step's own backward image goes with the forward one
        for i in (2, 4, 5):
            assert sum(_packs(trace[i], "_prepare_bwd").values()) == 1, (i, trace[i])
    # the guarantee itself: a new model given the trained weights computes the same bits
    for got, w, steps in ((outs[2], weights[0], 1), (outs[3], weights[2], 3)):
        ref = c.make()
        ref.set_keras_weights(w)
        got, want = _tensors(got), _tensors(c.forward(ref))
        assert len(got) == len(want) and all(torch.equal(a, b) for a, b in zip(got, want)), \
            f"the forward after {steps} step(s) differs from a new model's on the same weights"
