"""WideDeep.train_step / train_step_onehot (compile_fit on
model/wideDeep.py:47): BCE on sigmoid(0.5 (wide + deep)), WideLayer's l2 on
w, DNNLayer's Dropout in training mode, plain SGD.

The fp64 reference (wd_train_step) is plain numpy.  CPU tests pin it by
central finite differences of compile_fit's objective (step 1e-6, agreement
1e-6: the rule of test_train_blocks part A) including the l2 term, check
that the packed and the compact form agree to 1e-12, and assert the mask
precondition of every GPU case (see tests/test_deepcrossing_train.py): in the
reference every ReLU input z satisfies |z| > 1e-5 rms(z).  GPU tests follow
test_nfm_train_steps_match_oracle: three steps, lr 0.2, repeated rows in one
field, every weight after every step at assert_scaled_close 1e-5."""
import functools
import os

import numpy as np
import pytest
import torch

from tests.helpers import assert_scaled_close, criteo_columns, dropout_masks

gpu_test = pytest.mark.gpu
F64 = np.float64
F32 = np.float32
ND = 13


def _d(a):
    return np.asarray(a, F64)


# --------------------------------------------------------------------------
# fp64 reference
# --------------------------------------------------------------------------
def onehot(ids, offsets, widths):
    ids = np.asarray(ids).astype(np.int64)
    out = np.zeros((ids.shape[0], int(np.sum(widths))), F64)
    for c, (off, wid) in enumerate(zip(offsets, widths)):
        ok = (ids[:, c] >= 0) & (ids[:, c] < wid)
        out[np.nonzero(ok)[0], off + ids[ok, c]] = 1.0
    return out


def unpack(X, nd, F):
    """(wide input, codes) of the packed row [dense | codes | dense | dummies]."""
    X = _d(X)
    return np.concatenate([X[:, :nd], X[:, nd + F:]], axis=1), X[:, nd:nd + F].astype(np.int64)


def compact_inputs(dense, ids, offsets, widths):
    wide_in = np.concatenate([_d(dense), _d(dense), onehot(ids, offsets, widths)], axis=1)
    return wide_in, np.asarray(ids).astype(np.int64)


def wd_forward(wide_in, codes, p, masks=None):
    """Training-mode forward; returns (z, emb, acts, zs): acts[i] the input of
    layer i (after the dropout multiplier), zs the ReLU inputs."""
    wide = _d(p["w0"]).reshape(-1)[0] + wide_in @ _d(p["w"]).reshape(-1)
    emb = np.concatenate([_d(t)[codes[:, f]] for f, t in enumerate(p["tables"])], axis=1)
    acts, zs = [emb], []
    for i, (kern, bias) in enumerate(p["hidden"]):
        z = acts[-1] @ _d(kern) + _d(bias)
        zs.append(z)
        a = np.maximum(z, 0.0)
        if masks is not None:
            a = a * _d(masks[i])
        acts.append(a)
    deep = (acts[-1] @ _d(p["out"][0]) + _d(p["out"][1]))[:, 0]
    return 0.5 * (wide + deep), emb, acts, zs


def bce(z, t):
    return np.maximum(z, 0) - z * t + np.log1p(np.exp(-np.abs(z)))


def wd_objective(wide_in, codes, t, p, w_reg, masks=None):
    """compile_fit's objective: mean BCE + l2(w_reg) over every element of w."""
    return float(np.mean(bce(wd_forward(wide_in, codes, p, masks)[0], _d(t))) + w_reg * np.sum(_d(p["w"]) ** 2))


def wd_train_step(wide_in, codes, t, p, lr, w_reg, masks=None):
    """One SGD step; returns (new p, per-sample losses before the step, ReLU inputs)."""
    t = _d(t).reshape(-1)
    z, emb, acts, zs = wd_forward(wide_in, codes, p, masks)
    B = z.shape[0]
    g = (1.0 / (1.0 + np.exp(-z)) - t) / B
    gw = gd = 0.5 * g
    w = _d(p["w"]).reshape(-1, 1)
    new = {"w": w - lr * (wide_in.T @ gw[:, None] + 2.0 * w_reg * w), "w0": _d(p["w0"]).reshape(-1) - lr * gw.sum()}
    layers = [(_d(k), _d(b)) for k, b in p["hidden"]] + [(_d(p["out"][0]), _d(p["out"][1]))]
    nh = len(p["hidden"])
    delta, new_layers = gd[:, None], [None] * len(layers)
    for li in reversed(range(len(layers))):
        W, b = layers[li]
        new_layers[li] = (W - lr * (acts[li].T @ delta), b - lr * delta.sum(0))
        prev = delta @ W.T
        if 0 < li <= nh:
            prev = prev * (acts[li] > 0) if masks is None else prev * (zs[li - 1] > 0) * _d(masks[li - 1])
        delta = prev
    tables, c = [np.array(tb, F64) for tb in p["tables"]], 0
    for f, tb in enumerate(tables):
        k = tb.shape[1]
        np.add.at(tb, codes[:, f], -lr * delta[:, c:c + k])
        c += k
    new.update(tables=tables, hidden=new_layers[:nh], out=new_layers[nh])
    return new, bce(z, t), zs


def margins_ok(zs):
    return all(bool(np.all(np.abs(z) > 1e-5 * np.sqrt(np.mean(z ** 2)))) for z in zs)


# --------------------------------------------------------------------------
# cases
# --------------------------------------------------------------------------
CASES = {
    "small": dict(hidden=[64, 32], rate=0.0, B=37, seed=0),
    "small-drop": dict(hidden=[64, 32], rate=0.3, B=37, seed=0),
    "wide": dict(hidden=[256, 128, 64], rate=0.0, B=70, seed=2),
    "wide-drop": dict(hidden=[256, 128, 64], rate=0.3, B=70, seed=2),
}
F, K, LR, STEPS, W_REG, MODEL_SEED = 26, 8, 0.2, 3, 1e-3, 6


def _build(c, device):
    import recommender_system_amd as rs
    return rs.WideDeep(criteo_columns(c["vocabs"], n_dense=ND, embed_dim=K), c["hidden"], 1, "relu", embed_dim=K,
                       device=device, seed=MODEL_SEED, w_reg=W_REG)


def make_case(name, seed):
    """Initial weights, three batches in both forms, the dropout multipliers
    the model's generator draws (its seed depends on the model seed only), and
    the reference's trajectory."""
    from recommender_system_amd import models as M
    s = CASES[name]
    hidden, rate, B = s["hidden"], s["rate"], s["B"]
    rng = np.random.default_rng(seed)
    vocabs = [int(v) for v in rng.integers(2, 30, F)]
    widths = np.array(vocabs, np.int64)
    offsets = np.concatenate([[0], np.cumsum(widths)[:-1]])
    n = 2 * ND + int(widths.sum())
    dims = [F * K] + hidden
    glorot = lambda a, b: rng.uniform(-np.sqrt(6.0 / (a + b)), np.sqrt(6.0 / (a + b)), (a, b)).astype(F32)
    p0 = {"tables": [rng.normal(0, 0.5, (v, K)).astype(F32) for v in vocabs],
          "w": rng.normal(0, 0.05, (n, 1)).astype(F32), "w0": np.array([0.3], F32),
          "hidden": [(glorot(a, b), rng.normal(0, 0.05, b).astype(F32)) for a, b in zip(dims[:-1], dims[1:])],
          "out": (glorot(hidden[-1], 1), rng.normal(0, 0.05, 1).astype(F32))}
    c = dict(s, vocabs=vocabs, widths=widths, offsets=offsets, n=n, p0=p0)
    drop_seed, off = None, 0
    if rate:
        drop_seed = M._dropout_rng(_build(c, "cpu")).seed
    batches, traj, zs_all, p = [], [], [], p0
    for _ in range(STEPS):
        dense = rng.normal(0, 0.5, (B, ND)).astype(F32)
        ids = np.stack([rng.integers(0, v, B) for v in vocabs], 1).astype(np.int32)
        ids[:7, 3] = 0  # repeated rows
        t = rng.integers(0, 2, B).astype(F32)
        X = np.concatenate([dense, ids, dense, onehot(ids, offsets, widths)], axis=1).astype(F32)
        masks = None
        if rate:
            masks, off = dropout_masks(drop_seed, off, B, hidden, rate)
        wide_in, codes = unpack(X, ND, F)
        p, loss, zs = wd_train_step(wide_in, codes, t, p, LR, W_REG, masks)
        batches.append((dense, ids, t, X))
        traj.append((p, loss))
        zs_all += zs
    wide_in, codes = unpack(batches[-1][3], ND, F)
    c.update(batches=batches, traj=traj, zs=zs_all, final=1.0 / (1.0 + np.exp(-wd_forward(wide_in, codes, p)[0])))
    return c


@functools.lru_cache(maxsize=None)
def case(name):
    return make_case(name, CASES[name]["seed"])


# --------------------------------------------------------------------------
# CPU
# --------------------------------------------------------------------------
def _fd(f, x, h=1e-6):
    g = np.zeros_like(x)
    for idx in np.ndindex(x.shape):
        keep = x[idx]
        x[idx] = keep + h
        fp = f()
        x[idx] = keep - h
        fm = f()
        x[idx] = keep
        g[idx] = (fp - fm) / (2 * h)
    return g


def _fd_close(fd, g, what):
    g = _d(g)
    rms = float(np.sqrt(np.mean(g ** 2)))
    bad = ~(np.abs(fd - g) <= 1e-6 * np.maximum(np.abs(g), rms) + 1e-300)
    assert not bad.any(), f"{what}: finite differences off by {float(np.max(np.abs(fd - g))):.3e}"


def _tiny(rng):
    vocabs, k, hidden = [3, 2], 2, [4, 3]
    widths = np.array(vocabs)
    offsets = np.array([0, 3])
    n = 2 * 1 + 5
    dims = [len(vocabs) * k] + hidden
    p = {"tables": [rng.normal(0, 0.5, (v, k)) for v in vocabs], "w": rng.normal(0, 0.5, (n, 1)), "w0": np.array([0.3]),
         "hidden": [(rng.normal(0, 0.6, (a, b)), rng.normal(0, 0.1, b)) for a, b in zip(dims[:-1], dims[1:])],
         "out": (rng.normal(0, 0.6, (hidden[-1], 1)), np.array([0.05]))}
    dense = rng.normal(0, 0.5, (3, 1))
    ids = np.array([[0, 1], [2, 0], [0, 1]])  # row 0 of field 0 and row 1 of field 1 twice
    return p, dense, ids, offsets, widths, np.array([1.0, 0.0, 1.0])


@pytest.mark.parametrize("with_masks", [False, True])
def test_fd_widedeep_step(with_masks):
    """(p - p_new) / lr == central differences of mean BCE + w_reg |w|^2 for
    every weight (a visible l2 term: w_reg = 0.05), with and without fixed
    dropout multipliers."""
    rng = np.random.default_rng(3)
    p, dense, ids, offsets, widths, t = _tiny(rng)
    w_reg, lr = 0.05, 0.5
    masks = [np.array([[0, 2, 2, 0], [2, 2, 0, 2], [2, 0, 2, 2.0]]), np.array([[2, 0, 2], [0, 2, 2], [2, 2, 2.0]])] \
        if with_masks else None
    wide_in, codes = compact_inputs(dense, ids, offsets, widths)
    f = lambda: wd_objective(wide_in, codes, t, p, w_reg, masks)
    new, loss, zs = wd_train_step(wide_in, codes, t, p, lr, w_reg, masks)
    assert margins_ok(zs)
    np.testing.assert_allclose(np.mean(loss) + w_reg * np.sum(p["w"] ** 2), f(), rtol=1e-14)
    grad = lambda old, nw: (_d(old).reshape(_d(nw).shape) - _d(nw)) / lr
    _fd_close(_fd(f, p["w"]), grad(p["w"], new["w"]), "w")
    # the l2 term is there: without it the gradient of w differs visibly
    no_l2, _, _ = wd_train_step(wide_in, codes, t, p, lr, 0.0, masks)
    assert float(np.max(np.abs(no_l2["w"] - new["w"]))) > 1e-3
    # ... and reaches every element of w, also the one-hot columns no sample selects
    unused = 2 + 1  # field 0's code 1
    assert wide_in[:, unused].sum() == 0
    np.testing.assert_allclose(grad(p["w"], new["w"])[unused, 0], 2 * w_reg * p["w"][unused, 0], rtol=1e-12)
    _fd_close(_fd(f, p["w0"]), grad(p["w0"], new["w0"]), "w0")
    for c_, tb in enumerate(p["tables"]):
        _fd_close(_fd(f, tb), grad(tb, new["tables"][c_]), f"table {c_}")
    for l, ((kern, bias), (nk, nb)) in enumerate(zip(p["hidden"] + [p["out"]], new["hidden"] + [new["out"]])):
        _fd_close(_fd(f, kern), grad(kern, nk), f"W{l}")
        _fd_close(_fd(f, bias), grad(bias, nb), f"b{l}")


def test_packed_and_compact_forms_agree():
    rng = np.random.default_rng(5)
    p, dense, ids, offsets, widths, t = _tiny(rng)
    X = np.concatenate([dense, ids, dense, onehot(ids, offsets, widths)], axis=1)
    a, la, _ = wd_train_step(*unpack(X, 1, 2), t, p, 0.5, 0.05)
    b, lb, _ = wd_train_step(*compact_inputs(dense, ids, offsets, widths), t, p, 0.5, 0.05)
    assert float(np.max(np.abs(la - lb))) <= 1e-12
    for key in ("w", "w0"):
        assert float(np.max(np.abs(a[key] - b[key]))) <= 1e-12
    for x, y in zip(a["tables"] + [v for l in a["hidden"] + [a["out"]] for v in l],
                    b["tables"] + [v for l in b["hidden"] + [b["out"]] for v in l]):
        assert float(np.max(np.abs(x - y))) <= 1e-12


@pytest.mark.parametrize("name", sorted(CASES))
def test_mask_precondition(name):
    c = case(name)
    assert any((z < 0).any() for z in c["zs"])
    assert margins_ok(c["zs"]), f"case {name}: a ReLU input of the reference lies within 1e-5 rms of zero"
    assert all(np.isfinite(loss).all() for _, loss in c["traj"])


def test_train_steps_off_device():
    import recommender_system_amd as rs
    m = rs.WideDeep(criteo_columns([5, 3], n_dense=2), [4], 1, "relu", device="cpu", seed=0, w_reg=1e-3)
    assert m.wide.w_reg == 1e-3 and rs.WideLayer(device="cpu").w_reg == 1e-4
    with pytest.raises(NotImplementedError, match="WideDeep.train_step: training runs only on a HIP device"):
        m.train_step(np.zeros((2, 4)), np.zeros(2))
    with pytest.raises(NotImplementedError, match="WideDeep.train_step_onehot: training runs only on a HIP device"):
        m.train_step_onehot(np.zeros((2, 2)), np.zeros((2, 2)), [0, 5], [5, 3], np.zeros(2))


# --------------------------------------------------------------------------
# GPU
# --------------------------------------------------------------------------
def _keras(p):
    w = {f"embed_layer/embedding_{i}/embeddings": t for i, t in enumerate(p["tables"])}
    w["wide/w0"], w["wide/w"] = p["w0"], p["w"]
    for i, (kern, bias) in enumerate(p["hidden"]):
        w[f"deep/dense_{i}/kernel"], w[f"deep/dense_{i}/bias"] = kern, bias
    w["deep/dense_out/kernel"], w["deep/dense_out/bias"] = p["out"]
    return {n: np.asarray(v) for n, v in w.items()}


def _model(gpu, c):
    m = _build(c, gpu)
    m.set_keras_weights(_keras(c["p0"]))
    return m


def _assert_weights(m, p, what):
    ref = _keras(p)
    for n, v in m.keras_weights().items():
        assert_scaled_close(v, ref[n].reshape(tuple(v.shape)), 1e-5, f"{what} {n}")


@gpu_test
@pytest.mark.parametrize("name", sorted(CASES))
def test_widedeep_train_steps_match_reference(gpu, name):
    """Both input forms == wd_train_step over 3 steps (lr 0.2, w_reg 1e-3,
    repeated rows in one field; the dropout cases feed the reference the
    multipliers of helpers.dropout_masks): the losses and every weight after
    every step, the two forms against each other, then the inference forward."""
    from recommender_system_amd import models as M
    c = case(name)
    packed, compact = _model(gpu, c), _model(gpu, c)
    kw = dict(lr=LR, return_loss=True, dropout=c["rate"] if c["rate"] else False)
    off = 0
    for step, ((dense, ids, t, X), (p, ref_loss)) in enumerate(zip(c["batches"], c["traj"])):
        if c["rate"]:
            assert M._dropout_rng(packed).offset == off == M._dropout_rng(compact).offset
            off = dropout_masks(0, off, c["B"], c["hidden"], c["rate"])[1]
        la = packed.train_step(X, t, **kw)
        lb = compact.train_step_onehot(dense, ids, c["offsets"], c["widths"], t, **kw)
        assert_scaled_close(la, ref_loss, 1e-5, f"step {step} loss (packed)")
        assert_scaled_close(lb, ref_loss, 1e-5, f"step {step} loss (compact)")
        _assert_weights(packed, p, f"step {step} packed")
        _assert_weights(compact, p, f"step {step} compact")
        for (n, a), b in zip(packed.keras_weights().items(), compact.keras_weights().values()):
            assert_scaled_close(a, b, 2e-5, f"step {step} packed vs compact {n}")  # each within 1e-5 of the reference
    dense, ids, _, X = c["batches"][-1]
    assert_scaled_close(packed(X).reshape(-1), c["final"], 1e-5, "forward after training")
    assert_scaled_close(compact.forward_onehot(dense, ids, c["offsets"], c["widths"]).reshape(-1), c["final"], 1e-5,
                        "forward_onehot after training")


@gpu_test
def test_default_dropout_is_the_layers(gpu):
    """dropout=None applies DNNLayer's own rate (0.2), as under Keras' fit:
    the step differs from the dropout-free one."""
    c = case("small")
    a, b = _model(gpu, c), _model(gpu, c)
    _, _, t, X = c["batches"][0]
    a.train_step(X, t, lr=LR)
    b.train_step(X, t, lr=LR, dropout=False)
    assert not torch.equal(a.deep.hidden_layer[0].kernel, b.deep.hidden_layer[0].kernel)
    _assert_weights(b, c["traj"][0][0], "dropout=False")


@gpu_test
@pytest.mark.parametrize("form", ["packed", "compact"])
def test_bad_id_changes_nothing(gpu, form):
    c = case("small")
    m = _model(gpu, c)
    before = {n: v.detach().clone() for n, v in m.keras_weights().items()}
    dense, ids, t, X = c["batches"][0]
    bad = ids.copy()
    bad[5, 2] = c["vocabs"][2]
    with pytest.raises(IndexError):
        if form == "packed":
            Xb = X.copy()
            Xb[:, ND:ND + F] = bad
            m.train_step(Xb, t, lr=LR, dropout=False)
        else:
            m.train_step_onehot(dense, bad, c["offsets"], c["widths"], t, lr=LR, dropout=False)
    for n, v in m.keras_weights().items():
        assert torch.equal(v, before[n]), f"{n} changed by a refused step"


@gpu_test
def test_output_dim_and_activation_limits(gpu):
    import recommender_system_amd as rs
    cols = criteo_columns([5, 3], n_dense=2)
    X = np.zeros((2, 2 + 2 + 2 + 8), F32)
    with pytest.raises(NotImplementedError, match="output_dim 1"):
        rs.WideDeep(cols, [4], 2, "relu", device=gpu, seed=0).train_step(X, np.zeros(2))
    with pytest.raises(NotImplementedError, match="relu"):
        rs.WideDeep(cols, [4], 1, "sigmoid", device=gpu, seed=0).train_step(X, np.zeros(2))


@gpu_test
def test_compile_fit_widedeep_on_bundled_sample(gpu):
    """compile_fit (model/wideDeep.py:47) on the first 640 rows of the bundled
    Criteo sample, in the compact form with the embedding layer's vocab as the
    one-hot widths: the mean training loss is finite and falls."""
    import recommender_system_amd as rs
    from recommender_system_amd.dataset import criteo_compact, features_dict
    from recommender_system_amd.train import compile_fit
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "criteo_train_1w.txt.gz")
    dense, ids, label, _ = criteo_compact(path)
    m = rs.WideDeep(features_dict(path), [64, 32], 1, "relu", seed=2)
    hist = compile_fit(m, dense[:640], ids[:640], label[:640], batch_size=32, epochs=3, sgd=0.05)
    assert np.isfinite(hist).all() and hist[-1] < hist[0], hist
    assert m.wide.w.shape[0] == 2 * dense.shape[1] + sum(m.embed_layer.vocab_sizes)
