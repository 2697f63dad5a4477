"""Training PNN(use_fgcnn=True, train_fgcnn=True): the FGCNN conv stack's
backward (rs_fgcnn_conv_bwd), the product layers' backward past 64 fields
(rs_product_bwd / rs_product_w_grad), FGCNNLayer.backward and PNN.gradients /
PNN.train_step.

The fp64 references are restated here: fgcnn_bwd_ref (the conv stack's
backward) and pnn_fgcnn_grads_ref (the whole model's loss and gradients,
composed with tests.test_fgcnn.fgcnn_ref and the oracle's product layers and
BCE).  Both are pinned by central finite differences of the fp64 loss and by a
hand-computed case of the pool routing.  The CPU tests cover the references
and the argument checks (nothing is launched); the GPU tests compare kernels,
layer and model at the project's tolerance (tests.helpers.RTOL).  Every weight
is drawn here with numpy and loaded into the model, so the references'
preconditions (no clipped logit) are the same numbers on every machine."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import ctr_oracle as O
from recommender_system_amd import _lib
from tests.helpers import RTOL, _np, assert_scaled_close, criteo_columns, random_ids
from tests.test_fgcnn import DEFAULT, FGCNN_CASES, fgcnn_ref

gpu_test = pytest.mark.gpu
EPS = O.KERAS_EPS


# ------------------------------------------------------------ fp64 references
def _conv_forward(x, convs, pooling_width, dt):
    """Per layer (padded input, pre-bias conv sums [B,H,k,Cout], pooled map)."""
    saved = []
    for (w, b), pw in zip(convs, pooling_width):
        w = np.asarray(w, dt)
        kw, H = w.shape[0], x.shape[1]
        before = (kw - 1) // 2
        xp = np.pad(x, ((0, 0), (before, kw - 1 - before), (0, 0), (0, 0)))
        s = sum(np.einsum("bhdc,cn->bhdn", xp[:, t:t + H], w[t, 0]) for t in range(kw))
        Hp = H // pw
        B, k = x.shape[0], x.shape[2]
        mem = s[:, :Hp * pw].reshape(B, Hp, pw, k, -1)
        x = np.tanh(mem.max(axis=2) + np.asarray(b, dt))
        saved.append((xp, s, x))
    return saved


def fgcnn_bwd_ref(e, convs, pooling_width, dpooled, dt=np.float64):
    """Backward of the conv stack of FGCNNLayer on e [B, F, k] from dpooled =
    per layer dL/d(pooled map) [B, H', k, Cout] through that layer's
    recombination Dense alone.  Top down: the pooled gradient (+ the layer
    above's input gradient) goes to the first pool member attaining the
    maximum, times 1 - p^2; rows the pool drops get zero; db = sum dY, dW[t] =
    Xpad[t:t+H]^T dY, dX = the transposed convolution.  Returns (de [B, F, k],
    [(dW [kw,1,Cin,Cout], db)] per layer, [dY] per layer, the smallest
    winner-to-runner-up gap)."""
    x = np.asarray(e, dt)[..., None]
    saved = _conv_forward(x, convs, pooling_width, dt)
    grads, dys, carry, gap = [None] * len(convs), [None] * len(convs), 0.0, np.inf
    for i in reversed(range(len(convs))):
        w = np.asarray(convs[i][0], dt)
        pw, kw = pooling_width[i], w.shape[0]
        xp, s, p = saved[i]
        B, H, k, Cout = s.shape
        Hp, before = H // pw, (kw - 1) // 2
        g = (np.asarray(dpooled[i], dt) + carry) * (1.0 - p * p)
        mem = s[:, :Hp * pw].reshape(B, Hp, pw, k, Cout)
        win = mem.argmax(axis=2)                       # numpy: the first maximum
        if pw > 1:
            top2 = np.sort(mem, axis=2)[:, :, -2:]
            gap = min(gap, float((top2[:, :, 1] - top2[:, :, 0]).min()))
        dmem = np.zeros_like(mem)
        np.put_along_axis(dmem, win[:, :, None], g[:, :, None], axis=2)
        dY = np.zeros_like(s)
        dY[:, :Hp * pw] = dmem.reshape(B, Hp * pw, k, Cout)
        dW = np.stack([np.einsum("bhdc,bhdn->cn", xp[:, t:t + H], dY) for t in range(kw)])[:, None]
        dxp = np.zeros_like(xp)
        for t in range(kw):
            dxp[:, t:t + H] += np.einsum("bhdn,cn->bhdc", dY, w[t, 0])
        carry = dxp[:, before:before + H]
        grads[i], dys[i] = (dW, dY.sum(axis=(0, 1, 2))), dY
    return carry[..., 0], grads, dys, gap


def _forward(p, ids, mode, pw, dt):
    """PNN(use_fgcnn=True) forward on parameters p with everything the
    backward needs."""
    tables = [np.asarray(tb, dt) for tb in p["tables"]]
    k = tables[0].shape[1]
    emb = O.embed_layer(ids, tables, dt)
    B = emb.shape[0]
    emb = emb.reshape(B, -1, k)
    new, pooled = fgcnn_ref(emb, p["convs"], p["denses"], pw, dt)
    z = np.concatenate([emb, new], axis=1)
    parts = [z.reshape(B, -1)]
    if mode != "outer":
        parts.append(O.inner_product_layer(z, dt))
    if mode != "inner":
        parts.append(O.outer_product_layer(z, p["outer_W"], dt))
    acts = [np.concatenate(parts, 1)]
    pres = []
    for W, b in p["dnn_hidden"]:
        pres.append(acts[-1] @ np.asarray(W, dt) + np.asarray(b, dt))
        acts.append(np.maximum(pres[-1], 0))
    pre = (acts[-1] @ np.asarray(p["dnn_out"][0], dt) + np.asarray(p["dnn_out"][1], dt))[:, 0]
    return emb, new, pooled, z, acts, pres, pre


def pnn_fgcnn_loss(p, ids, t, mode, pw, dt=np.float64):
    return O.pnn_bce(_forward(p, ids, mode, pw, dt)[-1], t, dt)[0]


def pnn_fgcnn_grads_ref(p, ids, t, mode, pw, dt=np.float64):
    """The loss of the PNN loop (oracle.pnn_bce on the DNN logit) of
    PNN(use_fgcnn=True) and its gradient for every tensor, backpropagated by
    hand (formulas and pair order as oracle.pnn_train_step).  Returns (per-
    sample losses, grads, info): grads has "embed_rows" [B, F, k] (before the
    scatter), "convs" / "denses" / "dnn_hidden" lists of (dW, db), "dnn_out",
    "outer_W"; info has the logits, the smallest |relu pre-activation| and the
    smallest pool gap."""
    t = np.asarray(t, dt).reshape(-1)
    emb, new, pooled, z, acts, pres, pre = _forward(p, ids, mode, pw, dt)
    B, F, k = emb.shape
    nz = z.shape[1]
    _, loss = O.pnn_bce(pre, t, dt)
    ybar = t.mean()
    q = np.clip(pre, EPS, 1 - EPS)
    inside = (pre >= EPS) & (pre <= 1 - EPS)
    delta = np.where(inside, (-ybar / (q + EPS) + (1 - ybar) / (1 - q + EPS)) / B, 0.0)[:, None].astype(dt)
    layers = [(np.asarray(W, dt), np.asarray(b, dt)) for W, b in list(p["dnn_hidden"]) + [p["dnn_out"]]]
    dl = [None] * len(layers)
    for li in reversed(range(len(layers))):
        dl[li] = (acts[li].T @ delta, delta.sum(0))
        delta = delta @ layers[li][0].T
        if li > 0:
            delta = delta * (acts[li] > 0)
    g = {"dnn_hidden": dl[:-1], "dnn_out": dl[-1]}
    dz = delta[:, :nz * k].reshape(B, nz, k).copy()
    row, col = O.pair_indices(nz)
    P, off = len(row), nz * k
    if mode != "outer":
        dpi = delta[:, off:off + P]
        off += P
        for pi, (i, j) in enumerate(zip(row, col)):
            dz[:, i] += dpi[:, pi:pi + 1] * z[:, j]
            dz[:, j] += dpi[:, pi:pi + 1] * z[:, i]
    if mode != "inner":
        W = np.asarray(p["outer_W"], dt)
        dpo = delta[:, off:off + P]
        dW = np.zeros_like(W)
        for pi, (i, j) in enumerate(zip(row, col)):
            Wp, gp = W[:, pi, :], dpo[:, pi:pi + 1]
            dz[:, i] += gp * (z[:, j] @ Wp)
            dz[:, j] += gp * (z[:, i] @ Wp.T)
            dW[:, pi, :] = (gp * z[:, j]).T @ z[:, i]
        g["outer_W"] = dW
    dnew = dz[:, F:].reshape(B, -1)
    g["denses"], dpooled, c = [], [], 0
    relu_min = min(float(np.abs(a).min()) for a in pres)
    for (dk, db), pm in zip(p["denses"], pooled):
        dk = np.asarray(dk, dt)
        u = dk.shape[1]
        flat = pm.reshape(B, -1)
        relu_min = min(relu_min, float(np.abs(flat @ dk + np.asarray(db, dt)).min()))
        dpre = dnew[:, c:c + u] * (new.reshape(B, -1)[:, c:c + u] > 0)
        g["denses"].append((flat.T @ dpre, dpre.sum(0)))
        dpooled.append((dpre @ dk.T).reshape(pm.shape))
        c += u
    de, g["convs"], _, gap = fgcnn_bwd_ref(emb, p["convs"], pw, dpooled, dt)
    g["embed_rows"] = dz[:, :F] + de
    return loss, g, {"pre": pre, "relu_min": relu_min, "gap": gap}


def product_bwd_ref(z, delta, W, inner, dt=np.float64):
    """dz and dW of [flat | inner | outer] from the DNN's input gradient, by
    the loops of oracle.pnn_train_step."""
    z, delta = np.asarray(z, dt), np.asarray(delta, dt)
    B, F, k = z.shape
    row, col = O.pair_indices(F)
    P, off = len(row), F * k
    dz = delta[:, :F * k].reshape(B, F, k).copy()
    dW = None
    if inner:
        for pi, (i, j) in enumerate(zip(row, col)):
            dz[:, i] += delta[:, off + pi, None] * z[:, j]
            dz[:, j] += delta[:, off + pi, None] * z[:, i]
        off += P
    if W is not None:
        W = np.asarray(W, dt)
        dW = np.zeros_like(W)
        for pi, (i, j) in enumerate(zip(row, col)):
            Wp, gp = W[:, pi, :], delta[:, off + pi, None]
            dz[:, i] += gp * (z[:, j] @ Wp)
            dz[:, j] += gp * (z[:, i] @ Wp.T)
            dW[:, pi, :] = (gp * z[:, j]).T @ z[:, i]
    return dz.reshape(B, F * k), dW


# ------------------------------------------------------------- parameters
def _glorot(rng, *shape, fan=None):
    fi, fo = fan if fan else (shape[0], shape[-1])
    lim = np.sqrt(6.0 / (fi + fo))
    return rng.uniform(-lim, lim, size=shape).astype(np.float32)


def make_params(rng, vocabs, k, cfg, hidden, mode, out_bias=0.5, out_scale=0.1):
    """Every tensor of PNN(use_fgcnn=True) at Keras' initial scales, with the
    tables times 8 and W times 4 (O(1) products, visible row updates), small
    random biases, and the output layer scaled as
    test_pnn_train_steps_match_oracle does so the logits sit inside the loss's
    clip range."""
    F = len(vocabs)
    p = {"tables": [rng.uniform(-0.4, 0.4, size=(int(v), k)).astype(np.float32) for v in vocabs],
         "convs": [], "denses": []}
    H, cin = F, 1
    for cout, kw, maps, pw in zip(cfg["filters"], cfg["kernel_width"], cfg["dnn_maps"], cfg["pooling_width"]):
        p["convs"].append((_glorot(rng, kw, 1, cin, cout, fan=(kw * cin, kw * cout)),
                           rng.uniform(-0.1, 0.1, size=cout).astype(np.float32)))
        H //= pw
        p["denses"].append((_glorot(rng, H * k * cout, maps * H * k),
                            rng.uniform(-0.1, 0.1, size=maps * H * k).astype(np.float32)))
        cin = cout
    nz = F + sum(d[0].shape[1] for d in p["denses"]) // k
    P = nz * (nz - 1) // 2
    if mode != "inner":
        p["outer_W"] = (0.2 * rng.standard_normal((k, P, k))).astype(np.float32)
    n = nz * k + P * (2 if mode == "both" else 1)
    p["dnn_hidden"] = []
    for h in hidden:
        p["dnn_hidden"].append((_glorot(rng, n, h), rng.uniform(-0.1, 0.1, size=h).astype(np.float32)))
        n = h
    p["dnn_out"] = ((out_scale * _glorot(rng, n, 1)).astype(np.float32), np.full(1, out_bias, np.float32))
    return p


def to64(v):
    """The parameters (nested lists / tuples of arrays) as fresh fp64 arrays."""
    if isinstance(v, dict):
        return {n: to64(x) for n, x in v.items()}
    if isinstance(v, (list, tuple)):
        return type(v)(to64(x) for x in v)
    return np.array(v, np.float64)


TINY = dict(filters=[2, 3], kernel_width=[2, 3], dnn_maps=[1, 1], pooling_width=[2, 1])  # 5 rows: the pool drops one


def _tiny_case(seed=3):
    rng = np.random.default_rng(seed)
    vocabs = [4, 3, 5, 2, 4]
    p = to64(make_params(rng, vocabs, 4, TINY, [6, 4], "both"))
    ids = random_ids(rng, 3, vocabs)
    ids[1, 2] = ids[0, 2]  # a repeated row
    t = np.array([1.0, 0.0, 1.0])
    return p, ids, t


def _ints(v):
    return (C.c_int * len(v))(*v)


# ------------------------------------------------------------------ CPU
def test_pool_routing_known_answer():
    """H=3, k=1, one filter, kw=2, pw=2, by hand.  'same' pads nothing before
    and one row after (an even width), so the conv sums are [.5*1+.25*2,
    .5*2+.25*8, .5*8+0] = [1, 3, 4]; the pool sees rows 0-1, row 1 wins, row 2
    (the largest) is dropped and gets no gradient.  With dpooled = 1: dy =
    1 - tanh(3.1)^2 at row 1, db = dy, dW = [x_1, x_2] dy = [2, 8] dy, dX =
    [0, w_0, w_1] dy."""
    e = np.array([[[1.0], [2.0], [8.0]]])
    w = np.array([0.5, 0.25]).reshape(2, 1, 1, 1)
    de, grads, dys, gap = fgcnn_bwd_ref(e, [(w, [0.1])], [2], [np.ones((1, 1, 1, 1))])
    dy = 1 - np.tanh(3.1) ** 2
    assert np.allclose(dys[0].reshape(-1), [0, dy, 0], atol=1e-15)
    assert abs(gap - 2.0) < 1e-15
    assert np.allclose(grads[0][1], [dy], atol=1e-15)
    assert np.allclose(grads[0][0].reshape(-1), [2 * dy, 8 * dy], atol=1e-15)
    assert np.allclose(de.reshape(-1), [0, 0.5 * dy, 0.25 * dy], atol=1e-15)
    # a tie: sums [2, 2, 5] with w = [1, 0]; the FIRST maximum (row 0) takes the gradient
    e2 = np.array([[[2.0], [2.0], [5.0]]])
    w2 = np.array([1.0, 0.0]).reshape(2, 1, 1, 1)
    de2, g2, dys2, gap2 = fgcnn_bwd_ref(e2, [(w2, [0.0])], [2], [np.ones((1, 1, 1, 1))])
    dy2 = 1 - np.tanh(2.0) ** 2
    assert gap2 == 0.0
    assert np.allclose(dys2[0].reshape(-1), [dy2, 0, 0], atol=1e-15)
    assert np.allclose(de2.reshape(-1), [dy2, 0, 0], atol=1e-15)
    assert np.allclose(g2[0][0].reshape(-1), [2 * dy2, 2 * dy2], atol=1e-15)


FD_H = 1e-6


def test_references_match_finite_differences():
    """fgcnn_bwd_ref and pnn_fgcnn_grads_ref against central differences of
    the fp64 loss: 5 fields, k 4, conv widths 2 (even) and 3 (odd), a pool
    that drops a row, mode 'both', B 3, a repeated table row.  The loss has
    kinks (relus, the pool's winner, the logit clip); the seed is chosen so
    that every one of them is at least 100 FD steps away, which is asserted."""
    p, ids, t = _tiny_case()
    pw = TINY["pooling_width"]
    loss, g, info = pnn_fgcnn_grads_ref(p, ids, t, "both", pw)
    assert info["relu_min"] > 100 * FD_H and info["gap"] > 100 * FD_H
    assert info["pre"].min() > EPS + 100 * FD_H and info["pre"].max() < 1 - EPS - 100 * FD_H
    assert abs(loss.mean() - pnn_fgcnn_loss(p, ids, t, "both", pw)) < 1e-15
    # table gradients = the row gradients scattered
    dtab = [np.zeros_like(tb) for tb in p["tables"]]
    for c in range(len(dtab)):
        np.add.at(dtab[c], ids[:, c], g["embed_rows"][:, c])
    pairs = [(p["tables"][c], dtab[c], f"table {c}") for c in range(len(dtab))]
    for name in ("convs", "denses", "dnn_hidden"):
        for i, ((W, b), (dW, db)) in enumerate(zip(p[name], g[name])):
            pairs += [(W, dW.reshape(W.shape), f"{name}[{i}] kernel"), (b, db, f"{name}[{i}] bias")]
    pairs += [(p["dnn_out"][0], g["dnn_out"][0], "out kernel"), (p["dnn_out"][1], g["dnn_out"][1], "out bias"),
              (p["outer_W"], g["outer_W"], "outer W")]
    rng = np.random.default_rng(0)
    for arr, grad, what in pairs:
        assert arr.shape == grad.shape, what
        idx = rng.permutation(arr.size)[:40]  # every element of the small tensors, 40 of the large ones
        fd = np.empty(len(idx))
        for n, i in enumerate(idx):
            old = arr.flat[i]
            arr.flat[i] = old + FD_H
            up = pnn_fgcnn_loss(p, ids, t, "both", pw)
            arr.flat[i] = old - FD_H
            dn = pnn_fgcnn_loss(p, ids, t, "both", pw)
            arr.flat[i] = old
            fd[n] = (up - dn) / (2 * FD_H)
        ref = grad.flat[idx]
        scale = max(float(np.sqrt(np.mean(grad ** 2))), 1e-12)
        # central differences: O(h^2) truncation plus 1e-16 / h = 1e-10 of roundoff
        assert np.all(np.abs(fd - ref) <= 1e-5 * np.maximum(np.abs(ref), scale) + 1e-9), \
            f"{what}: max |fd - grad| {np.abs(fd - ref).max():.3e} at scale {scale:.3e}"


def test_new_entries_refuse_without_a_device():
    lib = _lib.lib()
    one = C.c_void_p(16)
    err = lib.rs_last_error_string
    # rs_product_bwd(z, z_stride, dx, dx_stride, F, k, inner, W, B, dz, dz_stride, stream)
    P = 26 * 25 // 2
    assert lib.rs_product_bwd(None, 208, one, 208 + 2 * P, 26, 8, 1, one, 4, one, 208, None) == -1
    assert b"rs_product_bwd: null" in err()
    assert lib.rs_product_bwd(one, 208, one, 208 + 2 * P, 26, 8, 1, one, 4, None, 208, None) == -1
    assert b"null" in err()
    assert lib.rs_product_bwd(one, 208, one, 208 + 2 * P, 26, 8, 0, None, 4, one, 208, None) == -1
    assert b"nothing to compute" in err()
    assert lib.rs_product_bwd(one, 207, one, 208 + 2 * P, 26, 8, 1, one, 4, one, 208, None) == -1
    assert b"stride" in err()
    assert lib.rs_product_bwd(one, 208, one, 208 + 2 * P - 1, 26, 8, 1, one, 4, one, 208, None) == -1
    assert b"stride" in err()
    assert lib.rs_product_bwd(one, 208, one, 208 + 2 * P, 26, 8, 1, one, 4, one, 207, None) == -1
    assert b"stride" in err()
    assert lib.rs_product_bwd(one, 129 * 8, one, 10 ** 6, 129, 8, 1, one, 4, one, 129 * 8, None) == -1
    assert b"2..128" in err()
    assert lib.rs_product_bwd(one, 26 * 32, one, 10 ** 6, 26, 32, 1, one, 4, one, 26 * 32, None) == -1
    assert b"k <= 16" in err()
    assert lib.rs_product_bwd(one, 208, one, 208 + 2 * P, 26, 8, 1, one, -1, one, 208, None) == -1
    assert lib.rs_product_bwd(None, 0, None, 0, 26, 8, 1, None, 0, None, 0, None) == 0  # an empty batch
    # rs_product_w_grad(z, z_stride, dx, dx_stride, F, k, inner, B, dW, stream)
    assert lib.rs_product_w_grad(one, 208, None, 208 + 2 * P, 26, 8, 1, 4, one, None) == -1
    assert b"rs_product_w_grad: null" in err()
    assert lib.rs_product_w_grad(one, 208, one, 208 + 2 * P, 26, 8, 1, 4, None, None) == -1
    assert lib.rs_product_w_grad(one, 208, one, 208 + P - 1, 26, 8, 0, 4, one, None) == -1
    assert b"stride" in err()
    assert lib.rs_product_w_grad(one, 129 * 8, one, 10 ** 6, 129, 8, 1, 4, one, None) == -1
    assert lib.rs_product_w_grad(one, 26 * 32, one, 10 ** 6, 26, 32, 1, 4, one, None) == -1
    assert lib.rs_product_w_grad(one, 208, one, 208 + 2 * P, 26, 8, 1, 0, one, None) == 0
    # rs_fgcnn_conv_bwd(z, zs, ws, wss, dws, dwss, F, k, L, filters, kw, pw, conv_w, de, des, dw, db, wsp, bytes, B, st)
    f, kw, pw = _ints([14, 16]), _ints([7, 7]), _ints([2, 2])
    ptrs = (C.c_void_p * 2)(16, 16)
    nul = (C.c_void_p * 2)(16, None)
    size = lib.rs_fgcnn_conv_bwd_workspace_size(26, 8, 2, f, kw, pw, 4)
    assert size == 4 * (7 * 14 + 14 + 7 * 14 * 16 + 16) * 4
    ok = dict(z=one, zs=208, ws=one, wss=2224, dws=one, dwss=2224, F=26, k=8, L=2, f=f, kw=kw, pw=pw, cw=ptrs, de=one,
              des=208, dw=ptrs, db=ptrs, wsp=one, nbytes=size, B=4, st=None)

    def bwd(**kwargs):
        return lib.rs_fgcnn_conv_bwd(*{**ok, **kwargs}.values())

    for name in ("z", "ws", "dws", "de", "cw", "dw", "db", "wsp"):
        assert bwd(**{name: None}) == -1 and b"rs_fgcnn_conv_bwd: null" in err(), name
    for name in ("cw", "dw", "db"):
        assert bwd(**{name: nul}) == -1 and b"null weights" in err(), name
    for name, v in (("zs", 207), ("des", 207), ("wss", 2223), ("dwss", 2223)):
        assert bwd(**{name: v}) == -1 and b"stride" in err(), name
    assert bwd(nbytes=size - 1) == -1 and b"workspace" in err()
    assert bwd(L=0) == -1 and b"layers" in err()
    assert bwd(k=6) == -1
    assert bwd(B=-1) == -1
    assert bwd(B=0) == 0


def test_conv_bwd_workspace_size():
    lib = _lib.lib()
    f, kw, pw = _ints([14, 16]), _ints([7, 7]), _ints([2, 2])
    row = (7 * 14 + 14 + 7 * 14 * 16 + 16) * 4
    assert lib.rs_fgcnn_conv_bwd_workspace_size(26, 8, 2, f, kw, pw, 1) == row
    assert lib.rs_fgcnn_conv_bwd_workspace_size(26, 8, 2, f, kw, pw, 0) == 0
    # the partial rows stop growing with the batch (one per workgroup)
    big = lib.rs_fgcnn_conv_bwd_workspace_size(26, 8, 2, f, kw, pw, 1 << 20)
    assert big == lib.rs_fgcnn_conv_bwd_workspace_size(26, 8, 2, f, kw, pw, 1 << 16) and big % row == 0
    for k in (8, 16, 32):  # the defaults fit
        assert lib.rs_fgcnn_conv_bwd_workspace_size(26, k, 2, f, kw, pw, 4) == 4 * row
    # k = 64: the forward's tile fits, the backward's (padded input + padded dY) does not
    assert lib.rs_fgcnn_workspace_size(26, 64, 2, f, kw, pw) > 0
    assert lib.rs_fgcnn_conv_bwd_workspace_size(26, 64, 2, f, kw, pw, 4) == -1
    assert b"LDS" in lib.rs_last_error_string()
    assert lib.rs_fgcnn_conv_bwd_workspace_size(26, 8, 0, f, kw, pw, 4) == -1
    assert lib.rs_fgcnn_conv_bwd_workspace_size(26, 8, 2, f, kw, pw, -1) == -1


def test_train_fgcnn_needs_use_fgcnn():
    from recommender_system_amd import PNN
    with pytest.raises(ValueError, match="use_fgcnn"):
        PNN(criteo_columns(np.full(26, 50)), "both", [8], 1, train_fgcnn=True, device="cpu")


# ------------------------------------------------------------------ GPU
def _t(a, dev, dtype=torch.float32):
    return torch.as_tensor(np.asarray(a)).to(dtype).to(dev).contiguous()


def _report(got, ref, what):
    got, ref = _np(got), _np(ref)
    rms = float(np.sqrt(np.mean(ref ** 2))) if ref.size else 0.0
    err = float(np.max(np.abs(got - ref) / np.maximum(np.maximum(np.abs(ref), rms), 1e-300))) if ref.size else 0.0
    print(f"[fgcnn_train] {what}: max scaled err {err:.3e}")


def close(got, ref, what):
    _report(got, ref, what)
    assert_scaled_close(got, ref, what=what)


def _run_product(z, delta, W, inner, gpu, pad=0):
    """rs_product_bwd + rs_product_w_grad on padded rows; returns (dz, dW)."""
    B, F, k = z.shape
    zt = torch.full((B, F * k + pad), 7.0, device=gpu)
    zt[:, :F * k] = _t(z.reshape(B, -1), gpu)
    dt_ = torch.full((B, delta.shape[1] + pad), 7.0, device=gpu)
    dt_[:, :delta.shape[1]] = _t(delta, gpu)
    dz = torch.full((B, F * k + pad), -7.0, device=gpu)
    Wt = None if W is None else _t(W, gpu)
    _lib.call("rs_product_bwd", zt.data_ptr(), zt.stride(0), dt_.data_ptr(), dt_.stride(0), F, k, 1 if inner else 0,
              None if Wt is None else Wt.data_ptr(), B, dz.data_ptr(), dz.stride(0), _lib.stream())
    assert bool((dz[:, F * k:] == -7.0).all())
    dW = None
    if Wt is not None:
        dW = torch.full_like(Wt, -7.0)
        _lib.call("rs_product_w_grad", zt.data_ptr(), zt.stride(0), dt_.data_ptr(), dt_.stride(0), F, k,
                  1 if inner else 0, B, dW.data_ptr(), _lib.stream())
    return dz[:, :F * k], dW


PRODUCT_CASES = [(2, 4, "both", 5), (26, 8, "both", 37), (26, 16, "outer", 5), (65, 4, "both", 5),
                 (83, 8, "both", 37), (83, 8, "inner", 5), (83, 8, "outer", 5), (83, 16, "both", 5),
                 (128, 8, "both", 37), (128, 16, "both", 5), (128, 4, "inner", 5)]


@gpu_test
@pytest.mark.parametrize("F,k,mode,B", PRODUCT_CASES)
def test_product_bwd(gpu, F, k, mode, B):
    """rs_product_bwd / rs_product_w_grad against the fp64 loops: 16 samples
    per workgroup (8 at F*k = 1024, 4 at 2048), ragged tiles (B 5, 37), padded
    row strides; bitwise reproducible; at F <= 64 also against the 64-field
    entries."""
    rng = np.random.default_rng(F * k + B)
    P = F * (F - 1) // 2
    inner, outer = mode != "outer", mode != "inner"
    z = rng.standard_normal((B, F, k)).astype(np.float32)
    W = (0.2 * rng.standard_normal((k, P, k))).astype(np.float32) if outer else None
    delta = rng.standard_normal((B, F * k + P * (inner + outer))).astype(np.float32)
    ref_dz, ref_dW = product_bwd_ref(z, delta, W, inner)
    dz, dW = _run_product(z, delta, W, inner, gpu, pad=3)
    dz2, dW2 = _run_product(z, delta, W, inner, gpu, pad=3)
    assert torch.equal(dz, dz2)
    close(dz, ref_dz, f"product dz F={F} k={k} {mode} B={B}")
    if outer:
        assert torch.equal(dW, dW2)
        close(dW, ref_dW, f"product dW F={F} k={k} {mode} B={B}")
    if F <= 64:
        zt, dl = _t(z.reshape(B, -1), gpu), _t(delta, gpu)
        w, st = dl.stride(0), _lib.stream()
        old = torch.empty(B, F * k, device=gpu)
        if inner:
            _lib.call("rs_inner_product_bwd", zt.data_ptr(), F * k, dl.data_ptr() + 4 * F * k, w, dl.data_ptr(), w, F, k,
                      B, old.data_ptr(), F * k, st)
        else:
            old.copy_(dl[:, :F * k])
        if outer:
            o0 = F * k + (P if inner else 0)
            Wt, oldW = _t(W, gpu), torch.empty(k, P, k, device=gpu)
            _lib.call("rs_outer_product_bwd", zt.data_ptr(), F * k, dl.data_ptr() + 4 * o0, w, Wt.data_ptr(), F, k, B,
                      old.data_ptr(), F * k, st)
            _lib.call("rs_outer_product_w_grad", zt.data_ptr(), F * k, dl.data_ptr() + 4 * o0, w, F, k, B,
                      oldW.data_ptr(), st)
            close(dW, oldW, "product dW against rs_outer_product_w_grad")
        close(dz, old, "product dz against the 64-field entries")


def _conv_layer(cfg, F, k, seed):
    """An FGCNNLayer with glorot kernels and random biases and its conv
    weights as the reference takes them."""
    from recommender_system_amd import FGCNNLayer
    layer = FGCNNLayer(**cfg, seed=seed)
    layer.build(F, k)
    rng = np.random.default_rng(seed)
    w = {n: v.cpu().numpy() for n, v in layer.keras_weights().items()}
    for n in w:
        if n.endswith("bias"):
            w[n] = rng.uniform(-0.3, 0.3, size=w[n].shape).astype(np.float32)
    layer.set_keras_weights(w)
    n = len(cfg["filters"])
    return layer, [(w[f"conv_{i}/kernel"], w[f"conv_{i}/bias"]) for i in range(n)], \
        [(w[f"dense_{i}/kernel"], w[f"dense_{i}/bias"]) for i in range(n)]


# The kernel finds the pool's winner from conv sums recomputed in fp32 (sums of
# at most 7 * 16 products of values below 1: rounding of some 1e-7, 1e-6 at the
# very worst), the reference in fp64.  A case whose closest pair of pool members is
# nearer than that could route a gradient to the other member in either
# arithmetic; the cases' seeds are chosen so none is, which each test asserts.
# The relu masks are taken from fp32 activations: the same holds for the
# smallest |pre-activation| of a model-level case (sums of up to 8,134 terms).
POOL_GAP = 4e-6
RELU_GAP = 5e-6

WIDE = dict(filters=[20, 32], kernel_width=[3, 2], dnn_maps=[1, 1], pooling_width=[2, 2])
CONV_BWD_CASES = FGCNN_CASES + [(9, 8, WIDE, 6)]


def _run_conv_bwd(layer, e_t, ws, dws, base, gpu):
    B, F, k = e_t.shape
    de = base.clone()
    dcw = [torch.full_like(w, -7.0) for w in layer.conv_kernels]
    dcb = [torch.full_like(b, -7.0) for b in layer.conv_biases]
    wsp = torch.empty(max(layer.bwd_workspace_size(B), 1), dtype=torch.uint8, device=gpu)
    _lib.call("rs_fgcnn_conv_bwd", e_t.data_ptr(), F * k, ws.data_ptr(), ws.stride(0), dws.data_ptr(), dws.stride(0),
              F, k, *layer._cfg(), _lib.ptrs(layer.conv_kernels), de.data_ptr(), de.stride(0), _lib.ptrs(dcw),
              _lib.ptrs(dcb), wsp.data_ptr(), wsp.numel(), B, _lib.stream())
    return de, dcw, dcb


@gpu_test
@pytest.mark.parametrize("F,k,cfg,B", CONV_BWD_CASES)
def test_fgcnn_conv_bwd(gpu, F, k, cfg, B):
    """rs_fgcnn_conv_bwd (dX_0 added into de, every dW and db) against
    fgcnn_bwd_ref on the forward's shapes, non-zero biases; bitwise
    reproducible."""
    layer, convs, _ = _conv_layer(cfg, F, k, seed=F * k + B)
    rng = np.random.default_rng(0)
    e = rng.standard_normal((B, F, k)).astype(np.float32)
    dws_np = rng.standard_normal((B, layer.ws_size)).astype(np.float32)
    dpooled, off = [], 0
    for H, kk, cout in layer.pooled_shapes:
        dpooled.append(dws_np[:, off:off + H * kk * cout].reshape(B, H, kk, cout))
        off += H * kk * cout
    base_np = rng.standard_normal((B, F * k)).astype(np.float32)
    ref_de, ref_g, _, gap = fgcnn_bwd_ref(e, convs, cfg["pooling_width"], dpooled)
    assert gap > POOL_GAP
    e_t, dws, base = _t(e, gpu), _t(dws_np, gpu), _t(base_np, gpu)
    ws = layer.conv(e_t)
    de, dcw, dcb = _run_conv_bwd(layer, e_t, ws, dws, base, gpu)
    de2, dcw2, dcb2 = _run_conv_bwd(layer, e_t, ws, dws, base, gpu)
    assert torch.equal(de, de2) and all(torch.equal(a, b) for a, b in zip(dcw + dcb, dcw2 + dcb2))
    close(de - base, ref_de.reshape(B, -1), f"conv bwd dX_0 F={F} k={k} B={B}")
    for i, (dW, db) in enumerate(ref_g):
        close(dcw[i], dW, f"conv bwd dW[{i}] F={F} k={k} B={B}")
        close(dcb[i], db, f"conv bwd db[{i}] F={F} k={k} B={B}")


@gpu_test
def test_fgcnn_conv_bwd_many_samples_per_workgroup(gpu):
    """B past the grid's 512 workgroups: workgroups take several samples and
    the last round is ragged."""
    cfg = dict(filters=[3], kernel_width=[2], dnn_maps=[1], pooling_width=[2])
    F, k, B = 5, 4, 1100
    layer, convs, _ = _conv_layer(cfg, F, k, seed=1)
    rng = np.random.default_rng(3)
    e = rng.standard_normal((B, F, k)).astype(np.float32)
    dws_np = rng.standard_normal((B, layer.ws_size)).astype(np.float32)
    ref_de, ref_g, _, gap = fgcnn_bwd_ref(e, convs, [2], [dws_np.reshape(B, 2, 4, 3)])
    assert gap > POOL_GAP
    e_t, dws, base = _t(e, gpu), _t(dws_np, gpu), torch.zeros(B, F * k, device=gpu)
    de, dcw, dcb = _run_conv_bwd(layer, e_t, layer.conv(e_t), dws, base, gpu)
    close(de, ref_de.reshape(B, -1), "conv bwd dX_0 B=1100")
    close(dcw[0], ref_g[0][0], "conv bwd dW B=1100")
    close(dcb[0], ref_g[0][1], "conv bwd db B=1100")


def _load(m, p):
    """The numpy parameters p into model m."""
    with torch.no_grad():
        e = m.embed_layer
        for c, tb in enumerate(p["tables"]):
            e.field_table(c).copy_(_t(tb, m._dev))
        fg = m.fgcnn_layer
        for i, ((w, b), (dk, db)) in enumerate(zip(p["convs"], p["denses"])):
            fg.conv_kernels[i].copy_(_t(w, m._dev))
            fg.conv_biases[i].copy_(_t(b, m._dev))
            fg.dense_layers[i].kernel.copy_(_t(dk, m._dev))
            fg.dense_layers[i].bias.copy_(_t(db, m._dev))
        if "outer_W" in p:
            m.outer_product_layer.W.copy_(_t(p["outer_W"], m._dev))
        for L, (W, b) in zip(list(m.dnn_layer.hidden_layer) + [m.dnn_layer.output_layer],
                             list(p["dnn_hidden"]) + [p["dnn_out"]]):
            L.kernel.copy_(_t(W, m._dev))
            L.bias.copy_(_t(b, m._dev))
    m._weights_changed()


def _named(m, g):
    """The reference's gradients under the model's parameter names."""
    out = {"embed_rows": g["embed_rows"]}
    for i, ((dW, db), (dk, dkb)) in enumerate(zip(g["convs"], g["denses"])):
        out[f"fgcnn_layer.conv_kernels.{i}"], out[f"fgcnn_layer.conv_biases.{i}"] = dW, db
        out[f"fgcnn_layer.dense_layers.{i}.kernel"], out[f"fgcnn_layer.dense_layers.{i}.bias"] = dk, dkb
    for i, (dW, db) in enumerate(g["dnn_hidden"]):
        out[f"dnn_layer.hidden_layer.{i}.kernel"], out[f"dnn_layer.hidden_layer.{i}.bias"] = dW, db
    out["dnn_layer.output_layer.kernel"], out["dnn_layer.output_layer.bias"] = g["dnn_out"]
    if "outer_W" in g:
        out["outer_product_layer.W"] = g["outer_W"]
    return out


def _model_case(mode, B, id_dtype, k=8, cfg=None, seed=0):
    from recommender_system_amd import PNN
    rng = np.random.default_rng(seed)
    vocabs = rng.integers(2, 300, size=26)
    fg = cfg or DEFAULT
    p = make_params(rng, vocabs, k, fg, [64, 32], mode)
    m = PNN(criteo_columns(vocabs, embed_dim=k), mode, [64, 32], 1, use_fgcnn=True, train_fgcnn=True, embed_dim=k,
            seed=1, fgcnn=cfg)
    _load(m, p)
    ids = random_ids(rng, B, vocabs, id_dtype)
    ids[:3, 4] = ids[0, 4]  # repeated rows in one field
    dense = rng.random((B, 13)).astype(np.float32)
    t = rng.integers(0, 2, B).astype(np.float32)
    if t.min() == t.max():
        t[0] = 1 - t[0]
    return m, p, vocabs, dense, ids, t


def _assert_unclipped(info):
    """Every logit inside the loss's clip range: a clipped one trains on zero
    gradient and shows nothing."""
    assert info["pre"].min() > 10 * EPS and info["pre"].max() < 1 - 10 * EPS, (info["pre"].min(), info["pre"].max())
    assert info["gap"] > POOL_GAP and info["relu_min"] > RELU_GAP


ONE_LAYER = dict(filters=[6], kernel_width=[4], dnn_maps=[2], pooling_width=[3])
# (the last entry: the first seed whose case keeps POOL_GAP and RELU_GAP)
GRAD_CASES = [("inner", 5, np.int32, 8, None, 0), ("outer", 5, np.int64, 8, None, 0), ("both", 5, np.int64, 8, None, 2),
              ("inner", 37, np.int64, 8, None, 66), ("outer", 37, np.int32, 8, None, 0),
              ("both", 37, np.int32, 8, None, 18), ("both", 5, np.int32, 4, ONE_LAYER, 0)]


@gpu_test
@pytest.mark.parametrize("mode,B,id_dtype,k,cfg,seed", GRAD_CASES)
def test_pnn_fgcnn_gradients(gpu, mode, B, id_dtype, k, cfg, seed):
    m, p, vocabs, dense, ids, t = _model_case(mode, B, id_dtype, k, cfg, seed)
    pw = (cfg or DEFAULT)["pooling_width"]
    loss_ref, g_ref, info = pnn_fgcnn_grads_ref(p, ids, t, mode, pw)
    _assert_unclipped(info)
    before = {n: v.clone() for n, v in m.named_parameters()}
    grads, loss = m.gradients((dense, ids), t)
    assert all(torch.equal(v, before[n]) for n, v in m.named_parameters())  # no weight moved
    want = _named(m, g_ref)
    assert set(grads) == set(want) == (set(before) - {"embed_layer.table"}) | {"embed_rows"}
    close(loss, loss_ref, f"{mode} B={B} losses")
    for n in sorted(want):
        assert tuple(grads[n].shape) == (tuple(before[n].shape) if n in before else (B, 26, k))
        close(grads[n], np.asarray(want[n]).reshape(tuple(grads[n].shape)), f"{mode} B={B} k={k} grad {n}")


def _ref_sgd(p, g, ids, lr):
    q = {"tables": [np.array(tb, np.float64) for tb in p["tables"]]}
    for c, tb in enumerate(q["tables"]):
        np.add.at(tb, ids[:, c], -lr * g["embed_rows"][:, c])
    for name in ("convs", "denses", "dnn_hidden"):
        q[name] = [(np.asarray(W, np.float64) - lr * dW.reshape(np.shape(W)), np.asarray(b, np.float64) - lr * db)
                   for (W, b), (dW, db) in zip(p[name], g[name])]
    q["dnn_out"] = (np.asarray(p["dnn_out"][0], np.float64) - lr * g["dnn_out"][0],
                    np.asarray(p["dnn_out"][1], np.float64) - lr * g["dnn_out"][1])
    if "outer_W" in p:
        q["outer_W"] = np.asarray(p["outer_W"], np.float64) - lr * g["outer_W"]
    return q


def _flat_params(p):
    out = {f"table {c}": tb for c, tb in enumerate(p["tables"])}
    for name in ("convs", "denses", "dnn_hidden"):
        for i, (W, b) in enumerate(p[name]):
            out[f"{name}[{i}] kernel"], out[f"{name}[{i}] bias"] = W, b
    out["out kernel"], out["out bias"] = p["dnn_out"]
    if "outer_W" in p:
        out["outer W"] = p["outer_W"]
    return {n: np.asarray(v, np.float64) for n, v in out.items()}


def _model_params(m):
    from tests.helpers import dnn_params, tables_of
    fg = m.fgcnn_layer
    c = lambda v: v.detach().cpu().numpy()
    hid, out = dnn_params(m.dnn_layer)
    p = {"tables": tables_of(m.embed_layer), "dnn_hidden": hid, "dnn_out": out,
         "convs": [(c(w), c(b)) for w, b in zip(fg.conv_kernels, fg.conv_biases)],
         "denses": [(c(d.kernel), c(d.bias)) for d in fg.dense_layers]}
    if m.mode != "inner":
        p["outer_W"] = c(m.outer_product_layer.W)
    return p


@gpu_test
def test_pnn_fgcnn_train_steps(gpu):
    """Two train_steps against the reference's SGD, comparing the UPDATES
    (after - before) of every tensor and of the touched table rows, the
    per-sample losses, and the forward on the trained weights.  An update is a
    difference of two stored fp32 weights, so beside RTOL on the update the
    bound carries one fp32 rounding of the weight it was added to (2^-24 |w|):
    that is the format's own limit for w - lr g, not a property of the
    kernels."""
    from tests.test_fgcnn import _pnn_ref
    mode, B, lr = "both", 37, 0.5
    m, p, vocabs, dense, ids, t = _model_case(mode, B, np.int64, seed=352)  # (both steps keep the gaps)
    pw = DEFAULT["pooling_width"]
    ref = to64(p)
    for step in range(2):
        loss_ref, g_ref, info = pnn_fgcnn_grads_ref(ref, ids, t, mode, pw)
        _assert_unclipped(info)
        new_ref = _ref_sgd(ref, g_ref, ids, lr)
        before = _flat_params(_model_params(m))
        loss = m.train_step((dense, ids), t, lr=lr, return_loss=True)
        after = _flat_params(_model_params(m))
        close(loss, loss_ref, f"step {step} losses")
        r0, r1 = _flat_params(ref), _flat_params(new_ref)
        for n in sorted(r1):
            upd, want = after[n] - before[n], r1[n] - r0[n]
            rms = float(np.sqrt(np.mean(want ** 2)))
            bound = RTOL * np.maximum(np.abs(want), rms) + 2.0 ** -24 * np.maximum(np.abs(before[n]), np.abs(after[n]))
            err = np.abs(upd - want)
            print(f"[fgcnn_train] step {step} update {n}: max err/bound {float(np.max(err / bound)):.3e}, "
                  f"rms {rms:.3e}")
            assert rms > 0 and np.all(err <= bound), f"step {step} update of {n}"
            if n.startswith("table"):  # only the looked-up rows moved
                c = int(n.split()[1])
                untouched = np.setdiff1d(np.arange(vocabs[c]), ids[:, c])
                assert not upd[untouched].any()
        ref = new_ref
    y_ref, _ = _pnn_ref(m, dense, ids, mode)
    close(m((dense, ids)), y_ref, "forward after training")


@gpu_test
def test_pnn_fgcnn_train_behaviour(gpu):
    from recommender_system_amd import PNN
    m, p, vocabs, dense, ids, t = _model_case("both", 9, np.int64, seed=1)
    # the default-built model keeps refusing; the message names the opt-in
    plain = PNN(criteo_columns(vocabs, embed_dim=8), "both", [64, 32], 1, use_fgcnn=True, embed_dim=8, seed=1)
    with pytest.raises(NotImplementedError, match="use_fgcnn.*train_fgcnn=True"):
        plain.train_step((dense, ids), t)
    with pytest.raises(NotImplementedError, match="use_fgcnn"):
        plain.gradients((dense, ids), t)
    with pytest.raises(ValueError, match="use_fgcnn"):
        PNN(criteo_columns(vocabs, embed_dim=8), "both", [64, 32], 1, train_fgcnn=True, embed_dim=8)
    # limits: raised before any launch
    for kw in (dict(embed_dim=32), dict(embed_dim=8, fgcnn=dict(dnn_maps=(12, 12)))):  # k 32; 26 + 228 fields
        big = PNN(criteo_columns(vocabs, embed_dim=kw["embed_dim"]), "inner", [8], 1, use_fgcnn=True, train_fgcnn=True,
                  seed=1, **kw)
        with pytest.raises(NotImplementedError, match="128 fields"):
            big.train_step((dense, ids), t)
    # a bad id raises with no weight changed
    before = {n: v.clone() for n, v in m.named_parameters()}
    bad = ids.copy()
    bad[2, 7] = vocabs[7]
    with pytest.raises(IndexError):
        m.train_step((dense, bad), t)
    with pytest.raises(IndexError):
        m.gradients((dense, bad), t)
    assert all(torch.equal(v, before[n]) for n, v in m.named_parameters())
    # B = 0: zero gradients, nothing moves
    g0, l0 = m.gradients((dense[:0], ids[:0]), t[:0])
    assert tuple(l0.shape) == (0,) and tuple(g0["embed_rows"].shape) == (0, 26, 8)
    assert all(not bool(v.any()) for v in g0.values())
    assert m.train_step((dense[:0], ids[:0]), t[:0]) is None
    assert all(torch.equal(v, before[n]) for n, v in m.named_parameters())
    # return_loss: the losses of gradients(), and every tensor moves
    _, loss = m.gradients((dense, ids), t)
    assert m.train_step((dense, ids), t) is None
    m2, *_ = _model_case("both", 9, np.int64, seed=1)
    assert torch.equal(m2.train_step((dense, ids), t, return_loss=True), loss)
    assert all(torch.equal(v, w) for v, w in zip(m.parameters(), m2.parameters()))
    assert all(not torch.equal(v, before[n]) for n, v in m.named_parameters())


@gpu_test
@pytest.mark.parametrize("mode", ["inner", "outer", "both"])
def test_pnn_plain_gradients_then_update_is_train_step(gpu, mode):
    """use_fgcnn=False: gradients followed by the manual update (one
    rs_sgd_update_multi, rs_embedding_sgd) equals train_step, bitwise."""
    from recommender_system_amd import PNN
    from recommender_system_amd._train_ops import embedding_sgd
    rng = np.random.default_rng(7)
    vocabs = rng.integers(2, 300, size=26)
    B, k, lr = 37, 8, 0.5
    make = lambda: PNN(criteo_columns(vocabs, embed_dim=k), mode, [64, 32], 1, embed_dim=k, seed=4)
    a, b = make(), make()
    for m in (a, b):
        with torch.no_grad():
            m.embed_layer.table.mul_(8.0)
            m.dnn_layer.output_layer.bias.fill_(0.5)
            m.dnn_layer.output_layer.kernel.mul_(0.1)
    ids = random_ids(rng, B, vocabs, np.int32)
    ids[:5, 4] = 0
    dense = rng.random((B, 13)).astype(np.float32)
    t = rng.integers(0, 2, B).astype(np.float32)
    loss_a = a.train_step((dense, ids), t, lr=lr, return_loss=True)
    before = {n: v.clone() for n, v in b.named_parameters()}
    grads, loss_b = b.gradients((dense, ids), t)
    assert all(torch.equal(v, before[n]) for n, v in b.named_parameters())
    assert torch.equal(loss_a, loss_b) and bool((loss_b > 0).all())
    assert set(grads) == (set(before) - {"embed_layer.table"}) | {"embed_rows"}
    assert tuple(grads["embed_rows"].shape) == (B, 26, k)
    names = dict(b.named_parameters())
    de = grads.pop("embed_rows").view(B, 26 * k)
    st = _lib.stream()
    _lib.sgd_update_multi([(names[n], g, g.numel(), 0.0) for n, g in grads.items()], lr, st)
    embedding_sgd(b.embed_layer, _t(ids, gpu, torch.int32), de.data_ptr(), 26 * k, lr, st, b)
    for n, w in a.named_parameters():
        assert torch.equal(w, names[n]), n
        assert not torch.equal(w, before[n]), n
