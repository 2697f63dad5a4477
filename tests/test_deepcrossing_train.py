"""Training the residual stack and DeepCrossing (compile_fit on
model/deepCrossing.py:45): the saved-activation forward
(rs_res_tower_train_fwd / rs_deepcrossing_train_fwd), the one-launch backward
data path (rs_res_tower_bwd) and DeepCrossing.train_step.

The fp64 references are plain numpy (stack_forward / stack_backward /
dc_train_step).  CPU tests pin them by central finite differences (a random
linear functional, step 1e-6, agreement 1e-6: the rule of test_train_blocks
part A), check the size queries against closed forms, the argument checks
with dummy pointers, and the MASK PRECONDITION of every GPU case: an fp32
kernel can be compared with an fp64 reference only if no ReLU flips, so in
the reference every ReLU input z of a layer satisfies |z| > 1e-5 rms(z) (the
margin of helpers.assert_scaled_close, inside which a passing forward cannot
change a sign).  The seeds below are chosen so the reference alone meets it;
a case that stops meeting it fails as a precondition, not as a tolerance.

GPU tests compare at the project's tolerance (helpers.RTOL) and check the
bit-exactness and determinism contracts of the ABI."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from recommender_system_amd import _lib
from tests.helpers import RTOL, assert_scaled_close, criteo_columns

gpu_test = pytest.mark.gpu
F64 = np.float64
F32 = np.float32


# --------------------------------------------------------------------------
# fp64 references
# --------------------------------------------------------------------------
def _d(a):
    return np.asarray(a, F64)


def stack_forward(x0, units):
    """The residual stack.  units: [(hidden [(kernel, bias)], out (kernel,
    bias))].  Returns xs (x_0 .. x_U), acts[u][l] (relu outputs of the hidden
    layers) and zs (every ReLU input, for the mask precondition)."""
    xs, acts, zs = [_d(x0)], [], []
    for hidden, out in units:
        a, au = xs[-1], []
        for kern, bias in hidden:
            z = a @ _d(kern) + _d(bias)
            zs.append(z)
            a = np.maximum(z, 0.0)
            au.append(a)
        z = xs[-1] + (a @ _d(out[0]) + _d(out[1]))
        zs.append(z)
        xs.append(np.maximum(z, 0.0))
        acts.append(au)
    return xs, acts, zs


def stack_backward(xs, acts, units, dy):
    """dy = dL/dx_U.  Returns deltas[u][l] = dL/d(pre-activation of layer l of
    unit u) (l = n_hidden: dL/dx_{u+1} [x_{u+1} > 0]), dL/dx_0 and
    grads[u][l] = (dW, db).  Masks: post-activation > 0."""
    U = len(units)
    deltas, grads = [None] * U, [None] * U
    dy = _d(dy)
    for u in reversed(range(U)):
        hidden, out = units[u]
        nh = len(hidden)
        Ws = [_d(k) for k, _ in hidden] + [_d(out[0])]
        ins = [xs[u]] + acts[u]
        dl = [None] * (nh + 1)
        dl[nh] = dy * (xs[u + 1] > 0)
        for l in range(nh, 0, -1):
            dl[l - 1] = (dl[l] @ Ws[l].T) * (acts[u][l - 1] > 0)
        dy = dl[nh] + dl[0] @ Ws[0].T
        deltas[u] = dl
        grads[u] = [(ins[l].T @ dl[l], dl[l].sum(0)) for l in range(nh + 1)]
    return deltas, dy, grads


def embed(ids, tables):
    return np.concatenate([_d(t)[np.asarray(ids)[:, f].astype(np.int64)] for f, t in enumerate(tables)], axis=1)


def dc_forward(dense, ids, p):
    x0 = np.concatenate([_d(dense), embed(ids, p["tables"])], axis=1)
    xs, acts, zs = stack_forward(x0, p["units"])
    z = xs[-1] @ _d(p["head"][0]).reshape(-1) + float(np.asarray(p["head"][1]).reshape(-1)[0])
    return xs, acts, zs, z


def bce(z, t):
    return np.maximum(z, 0) - z * t + np.log1p(np.exp(-np.abs(z)))


def dc_train_step(dense, ids, t, p, lr):
    """One SGD step of compile_fit on DeepCrossing (mean BCE on the sigmoid
    head's logit, no regulariser).  Returns (new p, per-sample losses before
    the step, the ReLU inputs)."""
    ids = np.asarray(ids).astype(np.int64)
    t = _d(t).reshape(-1)
    xs, acts, zs, z = dc_forward(dense, ids, p)
    B = z.shape[0]
    g = (1.0 / (1.0 + np.exp(-z)) - t) / B
    hk, hb = _d(p["head"][0]).reshape(-1, 1), _d(p["head"][1]).reshape(-1)
    _, dx0, grads = stack_backward(xs, acts, p["units"], g[:, None] * hk[:, 0][None, :])
    units = []
    for (hidden, out), gu in zip(p["units"], grads):
        layers = [(_d(k) - lr * dW, _d(b) - lr * db) for (k, b), (dW, db) in zip(list(hidden) + [out], gu)]
        units.append((layers[:-1], layers[-1]))
    nd = np.asarray(dense).shape[1]
    tables, c = [np.array(tb, F64) for tb in p["tables"]], nd
    for f, tb in enumerate(tables):
        k = tb.shape[1]
        np.add.at(tb, ids[:, f], -lr * dx0[:, c:c + k])
        c += k
    new = {"tables": tables, "units": units, "head": (hk - lr * (xs[-1].T @ g[:, None]), hb - lr * g.sum())}
    return new, bce(z, t), zs


def margins_ok(zs):
    return all(bool(np.all(np.abs(z) > 1e-5 * np.sqrt(np.mean(z ** 2)))) for z in zs)


# --------------------------------------------------------------------------
# cases
# --------------------------------------------------------------------------
def rand_units(rng, d, hidden, n_units):
    """Keras shapes: glorot kernels, N(0, 0.05) biases (float32)."""
    units = []
    for _ in range(n_units):
        dims = [d] + list(hidden) + [d]
        layers = []
        for kin, nout in zip(dims[:-1], dims[1:]):
            lim = np.sqrt(6.0 / (kin + nout))
            layers.append((rng.uniform(-lim, lim, (kin, nout)).astype(F32), rng.normal(0, 0.05, nout).astype(F32)))
        units.append((layers[:-1], layers[-1]))
    return units


# (d, hidden, units, batch) of the issue, d = nd + F * k, and a seed whose
# reference meets the mask precondition
SHAPES = {
    "A": dict(d=221, hidden=[256, 256], units=4, B=37, nd=13, F=26, k=8, seed=2),
    "B": dict(d=24, hidden=[8], units=1, B=1, nd=4, F=5, k=4, seed=0),
    "C": dict(d=272, hidden=[40, 300, 16], units=2, B=16, nd=16, F=32, k=8, seed=0),
    "D": dict(d=48, hidden=[64], units=3, B=33, nd=8, F=5, k=8, seed=0),
}


def make_kcase(name, seed):
    s = SHAPES[name]
    d, hidden, U, B, nd, F, k = (s[n] for n in ("d", "hidden", "units", "B", "nd", "F", "k"))
    assert d == nd + F * k
    rng = np.random.default_rng(seed)
    units = rand_units(rng, d, hidden, U)
    head = (rng.normal(0, 0.05, (d, 1)).astype(F32), np.array([0.1], F32))
    vocabs = [int(v) for v in rng.integers(2, 50, F)]
    tables = [rng.normal(0, 0.5, (v, k)).astype(F32) for v in vocabs]
    ids = np.stack([rng.integers(0, v, B) for v in vocabs], 1).astype(np.int64)
    dense = rng.normal(0, 0.5, (B, nd)).astype(F32)
    x = np.concatenate([dense, embed(ids, tables).astype(F32)], axis=1)  # x ~ N(0, 0.5)
    dy = rng.normal(0, 1, (B, d)).astype(F32)
    g = (rng.normal(0, 1, B) / B).astype(F32)
    xs, acts, zs = stack_forward(x, units)
    logit = xs[-1] @ _d(head[0]).reshape(-1) + 0.1
    c = dict(s, units=units, head=head, vocabs=vocabs, tables=tables, ids=ids, dense=dense, x=x, dy=dy, g=g, xs=xs,
             acts=acts, zs=zs, logit=logit, U=U)
    c["bwd_dy"] = stack_backward(xs, acts, units, dy)[:2]
    c["bwd_g"] = stack_backward(xs, acts, units, _d(g)[:, None] * _d(head[0]).reshape(-1)[None, :])[:2]
    return c


@functools.lru_cache(maxsize=None)
def kcase(name):
    return make_kcase(name, SHAPES[name]["seed"])


MODELS = {
    # the demo shape: 26 fields, k 8, nd 13, [256, 256], 4 units, B 37
    "demo": dict(nd=13, F=26, k=8, hidden=[256, 256], units=4, B=37, seed=55),
    "tiny": dict(nd=2, F=3, k=4, hidden=[8], units=1, B=1, seed=0),
}
LR, STEPS = 0.2, 3


def make_mcase(name, seed):
    """Initial weights, three batches (repeated rows in one field) and the
    reference's weights / losses / ReLU inputs after every step."""
    s = MODELS[name]
    nd, F, k, hidden, U, B = (s[n] for n in ("nd", "F", "k", "hidden", "units", "B"))
    d = nd + F * k
    rng = np.random.default_rng(seed)
    vocabs = [int(v) for v in rng.integers(3, 60, F)]
    p0 = {"tables": [rng.normal(0, 0.5, (v, k)).astype(F32) for v in vocabs], "units": rand_units(rng, d, hidden, U),
          "head": (rng.normal(0, 0.05, (d, 1)).astype(F32), np.array([0.1], F32))}
    batches, traj, zs_all, p = [], [], [], p0
    for _ in range(STEPS):
        dense = rng.normal(0, 0.5, (B, nd)).astype(F32)
        ids = np.stack([rng.integers(0, v, B) for v in vocabs], 1).astype(np.int32)
        ids[:7, 1] = 0  # repeated rows
        t = rng.integers(0, 2, B).astype(F32)
        p, loss, zs = dc_train_step(dense, ids, t, p, LR)
        batches.append((dense, ids, t))
        traj.append((p, loss))
        zs_all += zs
    # the inference forward on the trained weights
    final = 1.0 / (1.0 + np.exp(-dc_forward(batches[-1][0], batches[-1][1], p)[3]))
    return dict(s, d=d, vocabs=vocabs, p0=p0, batches=batches, traj=traj, zs=zs_all, final=final)


@functools.lru_cache(maxsize=None)
def mcase(name):
    return make_mcase(name, MODELS[name]["seed"])


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


def _units64(rng, d, hidden, n_units):
    return [([(_d(k), _d(b)) for k, b in hid], (_d(out[0]), _d(out[1])))
            for hid, out in rand_units(rng, d, hidden, n_units)]


def test_fd_stack_backward():
    rng = np.random.default_rng(4)
    d, hidden, U, B = 5, [4, 3], 3, 4
    units = _units64(rng, d, hidden, U)
    x = rng.normal(0, 1, (B, d))
    c = rng.normal(size=(B, d))
    f = lambda: float((c * stack_forward(x, units)[0][-1]).sum())
    xs, acts, zs = stack_forward(x, units)
    assert any((z < 0).any() for z in zs) and margins_ok(zs)
    deltas, dx0, grads = stack_backward(xs, acts, units, c)
    _fd_close(_fd(f, x), dx0, "dx0")
    for u, (hid, out) in enumerate(units):
        for l, (kern, bias) in enumerate(list(hid) + [out]):
            _fd_close(_fd(f, kern), grads[u][l][0], f"unit {u} dW{l}")
            _fd_close(_fd(f, bias), grads[u][l][1], f"unit {u} db{l}")
            # delta_{u,l} is the gradient of the layer's bias, sample by sample
            np.testing.assert_allclose(deltas[u][l].sum(0), grads[u][l][1], rtol=1e-14)


def test_fd_deepcrossing_step():
    """(p - p_new) / lr == central differences of compile_fit's objective
    (mean BCE), for every weight, with a row looked up twice."""
    rng = np.random.default_rng(9)
    nd, k, hidden, U, B = 1, 2, [3], 2, 3
    vocabs = [3, 2]
    d = nd + len(vocabs) * k
    p = {"tables": [rng.normal(0, 0.5, (v, k)) for v in vocabs], "units": _units64(rng, d, hidden, U),
         "head": (rng.normal(0, 0.3, (d, 1)), np.array([0.1]))}
    dense, t = rng.normal(0, 0.5, (B, nd)), np.array([1.0, 0.0, 1.0])
    ids = np.array([[0, 1], [2, 0], [0, 1]])
    f = lambda: float(np.mean(bce(dc_forward(dense, ids, p)[3], t)))
    new, loss, zs = dc_train_step(dense, ids, t, p, 0.5)
    assert margins_ok(zs)
    np.testing.assert_allclose(np.mean(loss), f(), rtol=1e-14)
    grad = lambda old, nw: (_d(old) - _d(nw)) / 0.5
    for c_, tb in enumerate(p["tables"]):
        _fd_close(_fd(f, tb), grad(tb, new["tables"][c_]), f"table {c_}")
    for u, (hid, out) in enumerate(p["units"]):
        nhid, nout = new["units"][u]
        for l, ((kern, bias), (nk, nb)) in enumerate(zip(list(hid) + [out], list(nhid) + [nout])):
            _fd_close(_fd(f, kern), grad(kern, nk), f"unit {u} W{l}")
            _fd_close(_fd(f, bias), grad(bias, nb), f"unit {u} b{l}")
    _fd_close(_fd(f, p["head"][0]), grad(p["head"][0], new["head"][0]), "head W")
    _fd_close(_fd(f, p["head"][1]), grad(p["head"][1], new["head"][1]), "head b")


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_mask_precondition_kernel_cases(name):
    c = kcase(name)
    assert any((z < 0).any() for z in c["zs"]) and any((z > 0).any() for z in c["zs"])
    assert margins_ok(c["zs"]), f"shape {name}: a ReLU input of the reference lies within 1e-5 rms of zero"


@pytest.mark.parametrize("name", sorted(MODELS))
def test_mask_precondition_model_cases(name):
    c = mcase(name)
    assert margins_ok(c["zs"]), f"model {name}: a ReLU input of the reference lies within 1e-5 rms of zero"
    assert all(np.isfinite(loss).all() for _, loss in c["traj"])


def _ints(v):
    return (C.c_int * max(len(v), 1))(*v)


def test_size_queries_closed_form():
    lib = _lib.lib()
    up = lambda v: (v + 15) // 16 * 16
    for d, hidden, U, B in [(221, [256, 256], 4, 37), (24, [8], 1, 1), (272, [40, 300, 16], 2, 16), (48, [64], 3, 0),
                            (1024, [1024] * 4, 16, 5)]:
        assert lib.rs_res_tower_ok(d, len(hidden), _ints(hidden), U) == 1
        assert lib.rs_res_tower_saved_size(d, len(hidden), _ints(hidden), U, B) == B * (d + U * (sum(hidden) + d))
        # the backward chain: d -> hidden reversed -> d, a bias slot per layer (zeros), the head slot
        dims = [d] + hidden[::-1] + [d]
        unit = sum(up(a) * up(b) + up(b) for a, b in zip(dims[:-1], dims[1:]))
        assert lib.rs_res_tower_bwd_prepared_size(d, len(hidden), _ints(hidden), U) == U * unit + up(d) + 16
        # ... the forward image's size: the same layers transposed
        assert lib.rs_res_tower_bwd_prepared_size(d, len(hidden), _ints(hidden), U) == \
            lib.rs_res_tower_prepared_size(d, len(hidden), _ints(hidden[::-1]), U, 1)
    for bad in [(221, [], 4), (221, [8] * 5, 4), (221, [256], 0), (221, [256], 17), (1025, [256], 1), (221, [1025], 1)]:
        d, hidden, U = bad
        assert lib.rs_res_tower_saved_size(d, len(hidden), _ints(hidden), U, 4) == -1
        assert b"rs_res_tower_saved_size" in lib.rs_last_error_string()
        assert lib.rs_res_tower_bwd_prepared_size(d, len(hidden), _ints(hidden), U) == -1
        assert b"rs_res_tower_bwd_prepared_size" in lib.rs_last_error_string()
    assert lib.rs_res_tower_saved_size(221, 1, _ints([8]), 1, -1) == -1


def test_argument_validation_without_device():
    lib = _lib.lib()
    p = C.c_void_p(16)
    h = _ints([8])
    err = lambda: lib.rs_last_error_string()
    # rs_res_tower_train_fwd(x, x_stride, d, nh, hidden, units, prepared, saved, out, logit, batch, stream)
    tf = lambda x=p, xs=20, nu=1, prep=p, saved=p, out=p, logit=p, B=4: lib.rs_res_tower_train_fwd(
        x, xs, 20, 1, h, nu, prep, saved, out, logit, B, None)
    for kw in ("x", "prep", "saved", "out", "logit"):
        assert tf(**{kw: None}) == -1 and b"rs_res_tower_train_fwd" in err() and b"null" in err(), kw
    assert tf(xs=19) == -1 and b"rs_res_tower_train_fwd" in err() and b"stride" in err()
    assert tf(nu=17) == -1 and b"rs_res_tower_train_fwd" in err()
    assert tf(B=-1) == -1 and b"rs_res_tower_train_fwd" in err()
    assert lib.rs_res_tower_train_fwd(None, 0, 20, 1, h, 1, None, None, None, None, 0, None) == 0
    # rs_deepcrossing_train_fwd: d = 4 + 2 * 8
    dc = lambda ids=p, kind=0, ids_s=2, dense=p, dense_s=4, table=p, saved=p, out=p, logit=p, B=4, nu=1: \
        lib.rs_deepcrossing_train_fwd(ids, kind, ids_s, dense, dense_s, 4, table, p, p, 2, 8, 1, h, nu, p, saved, out,
                                      logit, B, None, None)
    for kw in ("ids", "dense", "table", "saved", "out", "logit"):
        assert dc(**{kw: None}) == -1 and b"rs_deepcrossing_train_fwd" in err() and b"null" in err(), kw
    assert dc(kind=3) == -1 and b"id_kind" in err()
    assert dc(ids_s=1) == -1 and b"rs_deepcrossing_train_fwd" in err() and b"stride" in err()
    assert dc(dense_s=3) == -1 and b"stride" in err()
    assert dc(table=C.c_void_p(20)) == -1 and b"16-B aligned" in err()
    assert dc(nu=0) == -1 and b"rs_deepcrossing_train_fwd" in err()
    assert dc(ids=None, dense=None, table=None, saved=None, out=None, logit=None, B=0) == 0
    # rs_res_tower_prepare_bwd(d, nh, hidden, units, W, head_w, prepared, stream)
    assert lib.rs_res_tower_prepare_bwd(20, 1, h, 1, None, None, p, None) == -1
    assert b"rs_res_tower_prepare_bwd" in err() and b"null" in err()
    ws = (C.c_void_p * 2)(16, None)
    assert lib.rs_res_tower_prepare_bwd(20, 1, h, 1, ws, None, p, None) == -1 and b"layer 1" in err()
    ws = (C.c_void_p * 2)(16, 16)
    assert lib.rs_res_tower_prepare_bwd(20, 1, h, 1, ws, None, None, None) == -1 and b"null" in err()
    assert lib.rs_res_tower_prepare_bwd(20, 5, _ints([8] * 5), 1, ws, None, p, None) == -1
    assert b"rs_res_tower_prepare_bwd" in err()
    # rs_res_tower_bwd(saved, d, nh, hidden, units, image, dy, dy_stride, g, deltas, dx0, dx0_stride, batch, stream)
    bw = lambda saved=p, nu=1, img=p, dy=p, dys=20, g=None, deltas=p, dx0=p, dxs=20, B=4: lib.rs_res_tower_bwd(
        saved, 20, 1, h, nu, img, dy, dys, g, deltas, dx0, dxs, B, None)
    for kw in ("saved", "img", "deltas", "dx0"):
        assert bw(**{kw: None}) == -1 and b"rs_res_tower_bwd" in err() and b"null" in err(), kw
    assert bw(g=p) == -1 and b"exactly one" in err()
    assert bw(dy=None) == -1 and b"exactly one" in err()
    assert bw(dys=19) == -1 and b"rs_res_tower_bwd" in err() and b"stride" in err()
    assert bw(dxs=19) == -1 and b"stride" in err()
    assert bw(dy=None, dys=0, g=p, dxs=19) == -1 and b"stride" in err()
    assert bw(nu=17) == -1 and b"rs_res_tower_bwd" in err()
    assert bw(B=-1) == -1 and b"rs_res_tower_bwd" in err()
    assert bw(saved=None, img=None, dy=None, deltas=None, dx0=None, B=0) == 0


def test_train_step_off_device_and_bad_fused():
    import recommender_system_amd as rs
    m = rs.DeepCrossing(criteo_columns([5, 3], n_dense=2), 8, [4], 1, device="cpu", seed=0)
    with pytest.raises(NotImplementedError, match="DeepCrossing.train_step: training runs only on a HIP device"):
        m.train_step(np.zeros((2, 4)), np.zeros(2), fused=False)


# --------------------------------------------------------------------------
# GPU, kernel level
# --------------------------------------------------------------------------
SENT = -7.0


def _dev(a, gpu):
    return torch.as_tensor(np.ascontiguousarray(a), device=gpu)


def _arr(ts):
    return (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def _flat(units):
    return [l for hidden, out in units for l in list(hidden) + [out]]


def _padded(a, gpu, pad=3):
    """a [B, n] in a wider buffer with NaN in the padding; returns the view."""
    B, n = a.shape
    buf = torch.full((B, n + pad), float("nan"), dtype=torch.float32, device=gpu)
    buf[:, :n] = _dev(a, gpu)
    return buf[:, :n]


class Images:
    """The forward and backward images of a case's weights."""

    def __init__(self, c, gpu):
        lib = _lib.lib()
        d, hidden, U = c["d"], c["hidden"], c["U"]
        nh = len(hidden)
        self.keep = [(_dev(k, gpu), _dev(b, gpu)) for k, b in _flat(c["units"])]
        hw, hb = _dev(c["head"][0].reshape(-1), gpu), _dev(c["head"][1], gpu)
        self.keep.append((hw, hb))
        st = _lib.stream()
        n = lib.rs_res_tower_prepared_size(d, nh, _ints(hidden), U, 1)
        self.fwd = torch.full((n,), float("nan"), dtype=torch.float32, device=gpu)
        _lib.call("rs_res_tower_prepare", d, nh, _ints(hidden), U, _arr([k for k, _ in self.keep[:-1]]),
                  _arr([b for _, b in self.keep[:-1]]), hw.data_ptr(), hb.data_ptr(), self.fwd.data_ptr(), st)
        n = lib.rs_res_tower_bwd_prepared_size(d, nh, _ints(hidden), U)
        self.bwd = torch.full((n + 4,), float("nan"), dtype=torch.float32, device=gpu)
        self.bwd[n:] = SENT
        _lib.call("rs_res_tower_prepare_bwd", d, nh, _ints(hidden), U, _arr([k for k, _ in self.keep[:-1]]),
                  hw.data_ptr(), self.bwd.data_ptr(), st)
        torch.cuda.synchronize()
        assert not bool(torch.isnan(self.fwd).any())
        assert not bool(torch.isnan(self.bwd[:n]).any()), "rs_res_tower_prepare_bwd left part of the image unwritten"
        assert bool((self.bwd[n:] == SENT).all())


def _sizes(c, B):
    w = sum(c["hidden"]) + c["d"]
    return B * (c["d"] + c["U"] * w), B * c["U"] * w


def train_fwd(c, img, x, gpu):
    """rs_res_tower_train_fwd on the device view x; (saved, out, logit)."""
    B = x.shape[0]
    ns, _ = _sizes(c, B)
    saved = torch.full((ns + 4,), float("nan"), dtype=torch.float32, device=gpu)
    saved[ns:] = SENT
    out = torch.full((B + 1,), float("nan"), dtype=torch.float32, device=gpu)
    logit = torch.full((B + 1,), float("nan"), dtype=torch.float32, device=gpu)
    out[B], logit[B] = SENT, SENT
    _lib.call("rs_res_tower_train_fwd", x.data_ptr(), x.stride(0), c["d"], len(c["hidden"]), _ints(c["hidden"]), c["U"],
              img.fwd.data_ptr(), saved.data_ptr(), out.data_ptr(), logit.data_ptr(), B, _lib.stream())
    torch.cuda.synchronize()
    assert bool((saved[ns:] == SENT).all()) and float(out[B]) == SENT and float(logit[B]) == SENT
    return saved[:ns], out[:B], logit[:B]


def bwd(c, img, saved, gpu, dy=None, g=None):
    """rs_res_tower_bwd; (deltas, dx0 view of a wider buffer)."""
    d = c["d"]
    B = saved.numel() // (d + c["U"] * (sum(c["hidden"]) + d))
    _, nd_ = _sizes(c, B)
    deltas = torch.full((nd_ + 4,), float("nan"), dtype=torch.float32, device=gpu)
    deltas[nd_:] = SENT
    dx0 = torch.full((B, d + 3), float("nan"), dtype=torch.float32, device=gpu)
    dx0[:, d:] = SENT
    _lib.call("rs_res_tower_bwd", saved.data_ptr(), d, len(c["hidden"]), _ints(c["hidden"]), c["U"], img.bwd.data_ptr(),
              None if dy is None else dy.data_ptr(), 0 if dy is None else dy.stride(0),
              None if g is None else g.data_ptr(), deltas.data_ptr(), dx0.data_ptr(), dx0.stride(0), B, _lib.stream())
    torch.cuda.synchronize()
    assert bool((deltas[nd_:] == SENT).all()) and bool((dx0[:, d:] == SENT).all())
    return deltas[:nd_], dx0[:, :d]


def _split(flat, c, B, with_x0):
    """The tensors of saved / deltas: [x_0,] then per unit the layers' [B, N_l]."""
    widths = c["hidden"] + [c["d"]]
    out, o = [], 0
    if with_x0:
        out.append(flat[:B * c["d"]].view(B, c["d"]))
        o = B * c["d"]
    for u in range(c["U"]):
        for n in widths:
            out.append(flat[o:o + B * n].view(B, n))
            o += B * n
    assert o == flat.numel()
    return out


def _ref_saved(c):
    return [c["xs"][0]] + [t for u in range(c["U"]) for t in c["acts"][u] + [c["xs"][u + 1]]]


@gpu_test
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_train_fwd_saved_and_bit_exact(gpu, name):
    """saved against the fp64 reference at RTOL; out bit-identical to
    rs_res_tower_fwd(head 1), every saved x_{u+1} to rs_res_tower_fwd(head 0)
    with n_units = u + 1 on the same image; the ids form (int32, int64,
    float ids) bit-identical to the x form; a bad id sets the flag and stores
    a zero row."""
    c = kcase(name)
    img = Images(c, gpu)
    d, hidden, U, B, nd, F, k = (c[n] for n in ("d", "hidden", "U", "B", "nd", "F", "k"))
    nh, st = len(hidden), _lib.stream()
    x = _padded(c["x"], gpu)
    saved, out, logit = train_fwd(c, img, x, gpu)
    assert not bool(torch.isnan(saved).any()), "part of saved unwritten"
    got = _split(saved, c, B, True)
    for i, (a, r) in enumerate(zip(got, _ref_saved(c))):
        assert_scaled_close(a, r, RTOL, f"saved tensor {i}")
    assert_scaled_close(logit, c["logit"], RTOL, "logit")
    assert_scaled_close(out, 1.0 / (1.0 + np.exp(-c["logit"])), RTOL, "out")
    assert torch.equal(got[0], x)
    want = torch.empty(B, dtype=torch.float32, device=gpu)
    _lib.call("rs_res_tower_fwd", x.data_ptr(), x.stride(0), d, nh, _ints(hidden), U, img.fwd.data_ptr(), 1,
              want.data_ptr(), 1, B, st)
    assert torch.equal(out, want), "out differs from rs_res_tower_fwd(head 1)"
    for u in range(U):
        xu = torch.empty(B, d, dtype=torch.float32, device=gpu)
        _lib.call("rs_res_tower_fwd", x.data_ptr(), x.stride(0), d, nh, _ints(hidden), u + 1, img.fwd.data_ptr(), 0,
                  xu.data_ptr(), d, B, st)
        assert torch.equal(got[(u + 1) * (nh + 1)], xu), f"saved x_{u + 1} differs from rs_res_tower_fwd(head 0)"
    # the ids form
    tab = _dev(np.concatenate(c["tables"], axis=0), gpu)
    voc = torch.tensor(c["vocabs"], dtype=torch.int64, device=gpu)
    offs = torch.cumsum(voc, 0) - voc
    dense = _padded(c["dense"], gpu)
    ns, _ = _sizes(c, B)

    def ids_form(ids_np, dt):
        ids = _padded(ids_np.astype(dt), gpu) if dt == F32 else _dev(
            np.concatenate([ids_np, np.full((B, 2), -5)], axis=1).astype(dt), gpu)[:, :F]
        s2 = torch.full((ns,), float("nan"), dtype=torch.float32, device=gpu)
        o2, l2 = torch.empty(B, dtype=torch.float32, device=gpu), torch.empty(B, dtype=torch.float32, device=gpu)
        err = torch.zeros(1, dtype=torch.int32, device=gpu)
        _lib.call("rs_deepcrossing_train_fwd", ids.data_ptr(), _lib.id_kind(ids), ids.stride(0), dense.data_ptr(),
                  dense.stride(0), nd, tab.data_ptr(), offs.data_ptr(), voc.data_ptr(), F, k, nh, _ints(hidden), U,
                  img.fwd.data_ptr(), s2.data_ptr(), o2.data_ptr(), l2.data_ptr(), B, err.data_ptr(), st)
        torch.cuda.synchronize()
        return s2, o2, l2, int(err.item())

    bad = c["ids"].copy()
    bad[B - 1, F - 1] = c["vocabs"][F - 1]
    bad[0, 0] = -1
    xz = c["x"].copy()
    xz[B - 1, nd + (F - 1) * k:] = 0
    xz[0, nd:nd + k] = 0
    sz, oz, lz = train_fwd(c, img, _padded(xz, gpu), gpu)
    for dt in (np.int32, np.int64, F32):
        s2, o2, l2, flag = ids_form(c["ids"], dt)
        assert flag == 0
        assert torch.equal(s2, saved) and torch.equal(o2, out) and torch.equal(l2, logit), f"{dt.__name__} ids"
        s2, o2, l2, flag = ids_form(bad, dt)
        assert flag == _lib.FLAG_BAD_ID
        assert torch.equal(s2, sz) and torch.equal(o2, oz) and torch.equal(l2, lz), f"{dt.__name__} bad ids"


@gpu_test
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_bwd_vs_reference(gpu, name):
    """deltas and dx0 against the fp64 reference at RTOL in the dy and the g
    form, on the saved activations of the GPU forward; two runs bitwise equal;
    NaN in dy's padding, sentinels behind every output."""
    c = kcase(name)
    img = Images(c, gpu)
    B = c["B"]
    saved, _, _ = train_fwd(c, img, _padded(c["x"], gpu), gpu)
    for form in ("dy", "g"):
        kw = {"dy": _padded(c["dy"], gpu)} if form == "dy" else {"g": _dev(c["g"], gpu)}
        deltas, dx0 = bwd(c, img, saved, gpu, **kw)
        assert not bool(torch.isnan(deltas).any()) and not bool(torch.isnan(dx0).any()), "an output left unwritten"
        rd, rdx0 = c["bwd_" + form]
        ref = [t for u in range(c["U"]) for t in rd[u]]
        for i, (a, r) in enumerate(zip(_split(deltas, c, B, False), ref)):
            assert_scaled_close(a, r, RTOL, f"{form} form: delta tensor {i}")
        assert_scaled_close(dx0, rdx0, RTOL, f"{form} form: dx0")
        again, dx0b = bwd(c, img, saved, gpu, **kw)
        assert torch.equal(again, deltas) and torch.equal(dx0b, dx0), f"{form} form: two runs differ"


@gpu_test
@pytest.mark.parametrize("form", ["dy", "g"])
def test_bwd_batch_invariance(gpu, form):
    """The rows of batch 37 are bitwise equal to the same rows run as a batch
    of 5 taken from the middle (rows 14..18 span two tiles)."""
    c = kcase("A")
    img = Images(c, gpu)
    B, lo, hi = c["B"], 14, 19
    kw = lambda s: {"dy": _padded(c["dy"][s], gpu)} if form == "dy" else {"g": _dev(c["g"][s], gpu)}
    saved, _, _ = train_fwd(c, img, _dev(c["x"], gpu), gpu)
    deltas, dx0 = bwd(c, img, saved, gpu, **kw(slice(None)))
    sp, _, _ = train_fwd(c, img, _dev(c["x"][lo:hi], gpu), gpu)
    dp, dx0p = bwd(c, img, sp, gpu, **kw(slice(lo, hi)))
    for a, b in zip(_split(saved, c, B, True), _split(sp, c, hi - lo, True)):
        assert torch.equal(a[lo:hi], b), "saved rows depend on the batch"
    for a, b in zip(_split(deltas, c, B, False), _split(dp, c, hi - lo, False)):
        assert torch.equal(a[lo:hi], b), "delta rows depend on the batch"
    assert torch.equal(dx0[lo:hi], dx0p), "dx0 rows depend on the batch"


# --------------------------------------------------------------------------
# GPU, model level
# --------------------------------------------------------------------------
def _keras(p):
    w = {f"embed_layer/embedding_{i}/embeddings": t for i, t in enumerate(p["tables"])}
    for u, (hidden, out) in enumerate(p["units"]):
        for i, (kern, bias) in enumerate(hidden):
            w[f"res_layer_{u}/dense_{i}/kernel"], w[f"res_layer_{u}/dense_{i}/bias"] = kern, bias
        w[f"res_layer_{u}/dense_out/kernel"], w[f"res_layer_{u}/dense_out/bias"] = out
    w["output_layer/kernel"], w["output_layer/bias"] = p["head"]
    return {n: np.asarray(v) for n, v in w.items()}


def _model(gpu, c, seed=0):
    import recommender_system_amd as rs
    m = rs.DeepCrossing(criteo_columns(c["vocabs"], n_dense=c["nd"], embed_dim=c["k"]), 32, c["hidden"], c["units"],
                        embed_dim=c["k"], device=gpu, seed=seed)
    m.set_keras_weights(_keras(c["p0"]))
    return m


def _assert_weights(m, p, what):
    ref = _keras(p)
    for n, v in m.keras_weights().items():
        assert_scaled_close(v, ref[n].reshape(tuple(v.shape)), 1e-5, f"{what} {n}")


@gpu_test
@pytest.mark.parametrize("name,fused", [("demo", True), ("demo", False), ("tiny", True), ("tiny", False)])
def test_deepcrossing_train_steps_match_reference(gpu, name, fused):
    """DeepCrossing.train_step == dc_train_step over 3 steps (lr 0.2, repeated
    rows in one field): the losses and every weight after every step; then the
    inference forward on the trained weights."""
    c = mcase(name)
    m = _model(gpu, c)
    assert m.fused_ok()
    for step, ((dense, ids, t), (p, ref_loss)) in enumerate(zip(c["batches"], c["traj"])):
        loss = m.train_step((dense, ids), t, lr=LR, return_loss=True, fused=fused)
        assert_scaled_close(loss, ref_loss, 1e-5, f"step {step} loss")
        _assert_weights(m, p, f"step {step}")
    dense, ids, _ = c["batches"][-1]
    assert_scaled_close(m((dense, ids)).reshape(-1), c["final"], 1e-5, "forward after training")
    assert_scaled_close(m.forward_unfused((dense, ids)).reshape(-1), c["final"], 1e-5, "unfused forward after training")


@gpu_test
@pytest.mark.parametrize("fused", [True, False])
def test_bad_id_changes_nothing(gpu, fused):
    c = mcase("demo")
    m = _model(gpu, c)
    before = {n: v.detach().clone() for n, v in m.keras_weights().items()}
    dense, ids, t = c["batches"][0]
    bad = ids.copy()
    bad[5, 2] = c["vocabs"][2]
    with pytest.raises(IndexError):
        m.train_step((dense, bad), t, lr=LR, fused=fused)
    for n, v in m.keras_weights().items():
        assert torch.equal(v, before[n]), f"{n} changed by a refused step"
    # the model still trains
    m.train_step((dense, ids), t, lr=LR, fused=fused)
    _assert_weights(m, c["traj"][0][0], "step after a refused one")


@gpu_test
def test_fused_refused_where_the_kernels_do_not_take_the_shape(gpu):
    import recommender_system_amd as rs
    vocabs = [5, 30, 7]
    m = rs.DeepCrossing(criteo_columns(vocabs, n_dense=2), 32, [1100], 2, device=gpu, seed=0)
    assert not m.fused_ok()
    rng = np.random.default_rng(1)
    dense = rng.random((9, 2)).astype(F32)
    ids = np.stack([rng.integers(0, v, 9) for v in vocabs], 1)
    with pytest.raises(ValueError, match="fused=True"):
        m.train_step((dense, ids), np.zeros(9), fused=True)
    # fused=None falls back to the composition
    w0 = m.output_layer.kernel.detach().clone()
    loss = m.train_step((dense, ids), np.ones(9), lr=0.1, return_loss=True)
    assert bool(torch.isfinite(loss).all()) and not torch.equal(m.output_layer.kernel, w0)


@gpu_test
def test_train_step_graph_capture(gpu):
    """train_step(check_ids=False) captured once and replayed twice leaves the
    weights of two eager steps on a twin model, bit for bit (the step is a
    linear chain on one stream)."""
    c = mcase("demo")
    a, b = _model(gpu, c), _model(gpu, c)
    dense, ids, t = (_dev(v, gpu) for v in c["batches"][0])
    for m in (a, b):  # one eager step each: workspaces allocated outside the capture
        m.train_step((dense, ids), t, lr=0.05, check_ids=False, fused=True)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            a.train_step((dense, ids), t, lr=0.05, check_ids=False, fused=True)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    for _ in range(2):
        b.train_step((dense, ids), t, lr=0.05, check_ids=False, fused=True)
    torch.cuda.synchronize()
    wa, wb = a.keras_weights(), b.keras_weights()
    for n in wa:
        assert torch.equal(wa[n], wb[n]), f"{n}: replayed steps differ from eager steps"


@gpu_test
def test_compile_fit_deepcrossing_on_bundled_sample(gpu):
    """compile_fit (model/deepCrossing.py:45) on the first 640 rows of the
    bundled Criteo sample: the mean training loss is finite and falls."""
    import recommender_system_amd as rs
    from recommender_system_amd.dataset import criteo_compact, features_dict
    from recommender_system_amd.train import compile_fit
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "criteo_train_1w.txt.gz")
    dense, ids, label, _ = criteo_compact(path)
    m = rs.DeepCrossing(features_dict(path), 32, [32, 16], 2, seed=2)
    hist = compile_fit(m, dense[:640], ids[:640], label[:640], batch_size=32, epochs=3, sgd=0.05)
    assert np.isfinite(hist).all() and hist[-1] < hist[0], hist
