"""Training MMOE (mmoe_train.hip, MMOE.gradients / train_step / fit).

The fp64 restatement ``mmoe_train_ref`` follows include/rs_capi.h's "Training
MMOE" block and is pinned on the CPU by central finite differences of the
total loss (the l2 term included) and by a hand-computed case at E = 1.  The
CPU tests also cover the size / support queries against the header's closed
forms, the argument checks (dummy pointers, nothing launched) and the mask
precondition of every GPU case; the GPU tests compare every kernel output
block by block at tests.helpers.RTOL and check the bit-exactness contracts."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from recommender_system_amd import _lib
from tests.helpers import RTOL, assert_scaled_close
from tests.test_mmoe import TIMING, TOY, _ints, mmoe_ref, rand_weights, softmax_ref

gpu_test = pytest.mark.gpu
L2 = 1e-4
MMOE_LAYER = "mmoe_layer/"


# ------------------------------------------------------------ fp64 reference
class Ref:
    pass


def _tower_names(t, n_hidden):
    return [f"tower_layer_{t}/dense_{i}" for i in range(n_hidden)] + [f"tower_layer_{t}/dense_out"]


def mmoe_train_ref(x, labels, w, lr=0.01, loss_weights=None, act="relu", dt=np.float64):
    """One training step in ``dt`` arithmetic from Keras-named weights w and
    labels [T, B, Nout]: the saved blocks, losses, G, deltas, dz1, dx, the
    gradients (without l2), the total loss (with l2) and the new weights."""
    w = {k: np.asarray(v, dt) for k, v in w.items()}
    x, y = np.asarray(x, dt), np.asarray(labels, dt)
    em = w[MMOE_LAYER + "expert_matrix"]
    d, H, E = em.shape
    T, B, Nout = y.shape
    n_hidden = sum(1 for k in w if k.startswith("tower_layer_0/dense_") and k.endswith("/kernel")) - 1
    lw = np.ones(T, dt) if loss_weights is None else np.asarray(loss_weights, dt)
    r = Ref()
    eb, gb0 = w.get(MMOE_LAYER + "expert_bias"), w.get(MMOE_LAYER + "gate_bias0")
    r.pre_expert = x @ em.reshape(d, H * E) + (0 if eb is None else eb.reshape(-1))
    r.expert = np.maximum(r.pre_expert, 0)
    exp3 = r.expert.reshape(B, H, E)
    ps, mixes, acts, r.pre_hidden = [], [], [], [[] for _ in range(n_hidden)]
    r.z = np.zeros((T, B, Nout), dt)
    for t in range(T):
        logit = x @ w[MMOE_LAYER + f"gate_matrix{t}"] + (0 if gb0 is None else w[MMOE_LAYER + f"gate_bias{t}"])
        ps.append(softmax_ref(logit).astype(dt))
        mixes.append((exp3 * ps[t][:, None, :]).sum(-1))
        a = [mixes[t]]
        for i, n in enumerate(_tower_names(t, n_hidden)):
            zz = a[-1] @ w[n + "/kernel"] + w[n + "/bias"]
            if i < n_hidden:
                r.pre_hidden[i].append(zz)
                a.append(np.maximum(zz, 0) if act == "relu" else zz)
            else:
                r.z[t] = zz
        acts.append(a)
    r.gates, r.mix = np.concatenate(ps, 1), np.concatenate(mixes, 1)
    r.a = [np.concatenate([acts[t][i + 1] for t in range(T)], 1) for i in range(n_hidden)]
    r.loss = (np.maximum(r.z, 0) - r.z * y + np.log1p(np.exp(-np.abs(r.z)))).mean(-1)   # [T, B]
    reg = sum(float((v ** 2).sum()) for k, v in w.items() if k.startswith(MMOE_LAYER))
    r.total = float((lw * r.loss.mean(1)).sum()) + L2 * reg
    G = lw[:, None, None] * (1.0 / (1.0 + np.exp(-r.z)) - y) / (B * Nout)
    r.G = np.concatenate(list(G), 1)                                                     # [B, T Nout]
    # backward
    r.grads, dmix = {}, []
    deltas = [[None] * T for _ in range(n_hidden)]
    for t in range(T):
        delta = G[t]
        names = _tower_names(t, n_hidden)
        for l in reversed(range(n_hidden + 1)):
            r.grads[names[l] + "/kernel"] = acts[t][l].T @ delta
            r.grads[names[l] + "/bias"] = delta.sum(0)
            delta = delta @ w[names[l] + "/kernel"].T
            if l > 0:
                if act == "relu":
                    delta = delta * (acts[t][l] > 0)
                deltas[l - 1][t] = delta
        dmix.append(delta)
    r.deltas = [np.concatenate(dl, 1) for dl in deltas]
    dexp = sum(dmix[t][:, :, None] * ps[t][:, None, :] for t in range(T)) * (exp3 > 0)
    r.dp = [np.einsum("bh,bhe->be", dmix[t], exp3) for t in range(T)]
    r.gate_terms = np.concatenate([ps[t] * r.dp[t] for t in range(T)], 1)                # before the subtraction
    dlog = [ps[t] * (r.dp[t] - (ps[t] * r.dp[t]).sum(-1, keepdims=True)) for t in range(T)]
    r.dz1 = np.concatenate([dexp.reshape(B, H * E)] + dlog, 1)
    W1 = np.concatenate([em.reshape(d, H * E)] + [w[MMOE_LAYER + f"gate_matrix{t}"] for t in range(T)], 1)
    r.dx = r.dz1 @ W1.T
    gx = x.T @ r.dz1
    r.grads[MMOE_LAYER + "expert_matrix"] = gx[:, :H * E].reshape(d, H, E)
    if eb is not None:
        r.grads[MMOE_LAYER + "expert_bias"] = r.dz1[:, :H * E].sum(0).reshape(H, E)
    for t in range(T):
        cols = slice(H * E + t * E, H * E + (t + 1) * E)
        r.grads[MMOE_LAYER + f"gate_matrix{t}"] = gx[:, cols]
        if gb0 is not None:
            r.grads[MMOE_LAYER + f"gate_bias{t}"] = r.dz1[:, cols].sum(0)
    r.new = {k: v - lr * (r.grads[k] + (2 * L2 * v if k.startswith(MMOE_LAYER) else 0)) for k, v in w.items()}
    r.ps, r.n_hidden = ps, n_hidden
    return r


def fit_ref(x, labels, w, batch_size, epochs, lr, loss_weights, act="relu"):
    """compile_fit's loop on the reference step: (history, final weights)."""
    B, T = x.shape[0], labels.shape[0]
    lw = np.ones(T) if loss_weights is None else np.asarray(loss_weights, np.float64)
    w = {k: np.asarray(v, np.float64) for k, v in w.items()}
    hist = []
    for _ in range(epochs):
        tot = 0.0
        for b0 in range(0, B, batch_size):
            r = mmoe_train_ref(x[b0:b0 + batch_size], labels[:, b0:b0 + batch_size], w, lr, loss_weights, act)
            tot += float((lw[:, None] * r.loss).sum())
            w = r.new
        hist.append(tot / B)
    return hist, w


# ------------------------------------------------------------------- cases
class Case:
    pass


# name -> (configuration over TOY, batch, extras).  Seeds are chosen so that the
# fp64 reference alone meets the mask precondition (test_mask_precondition_cpu).
CASES = {
    "toy-B2": (dict(), 2, dict()),
    "toy-B19": (dict(), 19, dict()),
    "toy-B33": (dict(), 33, dict()),
    "timing-B33": (TIMING, 33, dict()),          # 8 chain tiles per layer: every wave owns whole tiles (S = 1)
    "E1": (dict(E=1), 19, dict()),
    "E16": (dict(E=16), 19, dict()),
    "T1": (dict(T=1), 19, dict()),
    "T8": (dict(T=8), 19, dict()),
    "H16": (dict(H=16), 19, dict()),
    "L1": (dict(towers=()), 19, dict()),
    "L3": (dict(towers=(20, 10, 7)), 19, dict()),
    "Nout2": (dict(out=2), 19, dict()),
    "nobias": (dict(), 19, dict(eb=False, gb=False)),
    "linear": (dict(), 19, dict(act="linear")),
    "xstride": (dict(), 19, dict(x_pad=5)),
    # T = 1, H = 10, towers (40,): the backward's layer 0 (W_0^T, [48 -> 16]) is ONE output tile of 3 k-groups,
    # mlp_slices(1, 3, 16) = 3: several k-slices per tile, met in LDS; dx (d 4: one tile of 3 k-groups) likewise
    "kslices": (dict(T=1, towers=(40,)), 19, dict()),
}


@functools.lru_cache(maxsize=None)
def make_case(name):
    over, B, extra = CASES[name]
    cfg = {**TOY, **over}
    c = Case()
    c.name, c.B = name, B
    c.d, c.H, c.E, c.T, c.towers, c.out = cfg["d"], cfg["H"], cfg["E"], cfg["T"], tuple(cfg["towers"]), cfg["out"]
    c.act, c.x_pad = extra.get("act", "relu"), extra.get("x_pad", 0)
    c.dims = [c.H, *c.towers, c.out]
    c.L = len(c.dims) - 1
    c.N1 = (c.H + c.T) * c.E
    rng = np.random.default_rng([7, sorted(CASES).index(name), B])
    c.w = rand_weights(rng, c.d, c.H, c.E, c.T, c.towers, c.out, extra.get("eb", True), extra.get("gb", True))
    c.x = rng.normal(0, 1, (B, c.d)).astype(np.float32)
    c.labels = rng.integers(0, 2, (c.T, B, c.out)).astype(np.float32)
    c.lw = [0.5 + 0.25 * t for t in range(c.T)]
    c.ref = mmoe_train_ref(c.x, c.labels, c.w, 0.01, c.lw, c.act)
    return c


def _rms(a):
    return float(np.sqrt(np.mean(np.asarray(a, np.float64) ** 2)))


def gate_close(got, ref, terms, what):
    """The gate part of dz1, p (dp - sum p dp), is a difference of like-sized
    terms: its error is set by the terms before the subtraction, so it is
    scaled by the rms of p_t[e] dp_t[e] (or its own size where larger), with
    the same RTOL."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, what
    bound = RTOL * np.maximum(np.abs(ref), _rms(terms)) + 1e-30
    err = np.abs(got - ref)
    assert (err <= bound).all(), f"{what}: max err / bound {float((err / bound).max()):.3e}"


# --------------------------------------------------------------------- CPU
def _fd_dir(f, arrs, dirs, h=1e-6):
    """Central difference of f() along `dirs` applied to `arrs` in place."""
    keep = [a.copy() for a in arrs]
    for a, k, u in zip(arrs, keep, dirs):
        a[...] = k + h * u
    fp = f()
    for a, k, u in zip(arrs, keep, dirs):
        a[...] = k - h * u
    fm = f()
    for a, k in zip(arrs, keep):
        a[...] = k
    return (fp - fm) / (2 * h)


@pytest.mark.parametrize("over,act", [(dict(), "relu"), (dict(out=2, towers=(6,)), "linear"), (dict(towers=()), "relu"),
                                      (dict(E=2, T=2), "relu")])
def test_reference_finite_differences(over, act):
    """d L / d(parameter group) and d L / dx of the reference against central
    differences of its own total loss (l2 included) along a random direction
    per group: step 1e-6, agreement 1e-6 (test_train_blocks.py part A: the
    error against max(|value|, the group's rms scale |g| |u| / sqrt(n)))."""
    cfg = {**TOY, **over}
    rng = np.random.default_rng(5)
    T = cfg["T"]
    w = {k: v.astype(np.float64) for k, v in
         rand_weights(rng, cfg["d"], cfg["H"], cfg["E"], T, cfg["towers"], cfg["out"]).items()}
    x = rng.normal(0, 1, (6, cfg["d"]))
    y = rng.integers(0, 2, (T, 6, cfg["out"])).astype(np.float64)
    lw = [0.5 + 0.25 * t for t in range(T)]
    r = mmoe_train_ref(x, y, w, 0.01, lw, act)
    if act == "relu":  # no kink within the step
        pre = [r.pre_expert] + [np.concatenate(p, 1) for p in r.pre_hidden]
        assert all(np.abs(p).min() > 2e-5 for p in pre)
    f = lambda: mmoe_train_ref(x, y, w, 0.01, lw, act).total
    groups = {"expert_matrix": ["mmoe_layer/expert_matrix"], "expert_bias": ["mmoe_layer/expert_bias"],
              "gate_matrix": [f"mmoe_layer/gate_matrix{t}" for t in range(T)],
              "gate_bias": [f"mmoe_layer/gate_bias{t}" for t in range(T)],
              "tower kernels": [k for k in w if k.startswith("tower") and k.endswith("kernel")],
              "tower biases": [k for k in w if k.startswith("tower") and k.endswith("bias")]}
    for what, names in groups.items():
        dirs = [rng.normal(size=w[n].shape) for n in names]
        full = [r.grads[n] + (2 * L2 * w[n] if n.startswith(MMOE_LAYER) else 0) for n in names]
        want = sum(float((g * u).sum()) for g, u in zip(full, dirs))
        scale = np.sqrt(sum((g ** 2).sum() for g in full) * sum((u ** 2).sum() for u in dirs) / sum(g.size for g in full))
        fd = _fd_dir(f, [w[n] for n in names], dirs)
        assert abs(fd - want) <= 1e-6 * max(abs(want), scale), f"{what}: fd {fd!r} vs {want!r}"
    u = rng.normal(size=x.shape)
    want = float((r.dx * u).sum())
    fd = _fd_dir(f, [x], [u])
    assert abs(fd - want) <= 1e-6 * max(abs(want), np.linalg.norm(r.dx) * np.linalg.norm(u) / np.sqrt(u.size))


def test_reference_known_answers_e1():
    """E = 1, d 2, H 2, T 2, no hidden layer, B = 1, x = [1, 2], by hand.
    Experts: x @ [[1, -1], [0.5, 0]] + [0, 0.5] = [2, -0.5] -> relu [2, 0];
    every gate is exactly 1, so mix_t = expert and the gate gradients are
    exactly 0.  Tower t: z_t = mix . k_t + b_t with k_0 = [1, 3], b_0 = -2 ->
    z_0 = 0; k_1 = [0.5, 1], b_1 = 0 -> z_1 = 1.  Labels [1, 0], weights [1,
    2]: G_0 = 1 (0.5 - 1) = -0.5, G_1 = 2 sigmoid(1).  dmix_t = G_t k_t;
    dexp = [G_0 + 0.5 G_1, 0] (the second expert is off)."""
    w = {"mmoe_layer/expert_matrix": np.array([[[1.0], [-1.0]], [[0.5], [0.0]]]),
         "mmoe_layer/expert_bias": np.array([[0.0], [0.5]]),
         "mmoe_layer/gate_matrix0": np.array([[0.3], [-0.2]]), "mmoe_layer/gate_matrix1": np.array([[1.5], [0.1]]),
         "mmoe_layer/gate_bias0": np.array([5.0]), "mmoe_layer/gate_bias1": np.array([-7.0]),
         "tower_layer_0/dense_out/kernel": np.array([[1.0], [3.0]]), "tower_layer_0/dense_out/bias": np.array([-2.0]),
         "tower_layer_1/dense_out/kernel": np.array([[0.5], [1.0]]), "tower_layer_1/dense_out/bias": np.array([0.0])}
    x, y = np.array([[1.0, 2.0]]), np.array([[[1.0]], [[0.0]]])
    r = mmoe_train_ref(x, y, w, 0.1, [1.0, 2.0])
    s1 = 1 / (1 + np.exp(-1.0))
    np.testing.assert_array_equal(r.expert, [[2.0, 0.0]])
    np.testing.assert_array_equal(r.gates, [[1.0, 1.0]])
    np.testing.assert_array_equal(r.mix, [[2.0, 0.0, 2.0, 0.0]])
    np.testing.assert_allclose(r.z[:, 0, 0], [0.0, 1.0], rtol=1e-15)
    np.testing.assert_allclose(r.loss[:, 0], [np.log(2.0), 1.0 + np.log1p(np.exp(-1.0))], rtol=1e-15)
    np.testing.assert_allclose(r.G, [[-0.5, 2 * s1]], rtol=1e-15)
    g = -0.5 + 0.5 * 2 * s1
    np.testing.assert_allclose(r.dz1, [[g, 0.0, 0.0, 0.0]], rtol=1e-15, atol=0)
    assert np.all(r.dz1[:, 2:] == 0) and np.all(r.grads["mmoe_layer/gate_matrix0"] == 0)
    assert np.all(r.grads["mmoe_layer/gate_bias1"] == 0)
    np.testing.assert_allclose(r.dx, [[g, 0.5 * g]], rtol=1e-15)
    np.testing.assert_allclose(r.grads["mmoe_layer/expert_matrix"][:, :, 0], [[g, 0.0], [2 * g, 0.0]], rtol=1e-15)
    np.testing.assert_allclose(r.grads["tower_layer_1/dense_out/kernel"][:, 0], [4 * s1, 0.0], rtol=1e-15)
    np.testing.assert_allclose(r.grads["tower_layer_0/dense_out/bias"], [-0.5], rtol=1e-15)
    # the step: l2 on the layer's tensors (gate_bias0: zero gradient, 5 -> 5 - 0.1 * 2e-4 * 5), none on the towers
    np.testing.assert_allclose(r.new["mmoe_layer/gate_bias0"], [5.0 - 0.1 * 2e-4 * 5.0], rtol=1e-15)
    np.testing.assert_allclose(r.new["tower_layer_0/dense_out/bias"], [-2.0 + 0.05], rtol=1e-15)
    np.testing.assert_allclose(r.total, np.log(2.0) + 2 * (1.0 + np.log1p(np.exp(-1.0)))
                               + 1e-4 * sum(float((v ** 2).sum()) for k, v in w.items() if k.startswith("mmoe")),
                               rtol=1e-15)
    # the forward half agrees with the forward's own restatement
    mix, yy = mmoe_ref(x, w, 2, 0)
    np.testing.assert_array_equal(mix, r.mix)
    np.testing.assert_allclose(yy, r.z, rtol=1e-15)


def _up(v, m=16):
    return (v + m - 1) // m * m


def expected_ok(d, H, E, T, dims):
    """rs_mmoe_ok's closed form (include/rs_capi.h)."""
    L = len(dims) - 1
    if not (1 <= d <= 1024 and 1 <= H <= 1024 and 1 <= E <= 16 and 1 <= T <= 8 and 0 <= L <= 4):
        return False
    if _up((H + T) * E) > 1024 or any(not 1 <= v <= 1024 for v in dims) or dims[0] != H:
        return False
    maxw = max([_up(d), E * (H | 1) + T * E] + [T * _up(v) for v in dims])
    return 4 * (32 * (_up(maxw, 64) + 8) + 4096) <= 160 * 1024


def expected_train_ok(d, H, E, T, dims):
    L = len(dims) - 1
    if L < 1 or not expected_ok(d, H, E, T, dims):
        return False
    maxw = max([_up(d), _up((H + T) * E)] + [T * _up(v) for v in dims])
    return 4 * (48 * (_up(maxw, 64) + 8) + 4096) <= 160 * 1024


def expected_saved_size(H, E, T, dims, B):
    return B * (H * E + T * E + T * H + T * sum(dims[1:-1]))


def expected_bwd_prepared_size(d, H, E, T, dims):
    return sum(T * _up(a) * _up(b) for a, b in zip(dims[:-1], dims[1:])) + _up((H + T) * E) * _up(d)


def test_size_queries_cpu():
    lib = _lib.lib()
    seen = {True: 0, False: 0}
    for d in (1, 4, 221, 1024):
        for H in (1, 10, 40, 64):
            for E in (1, 3, 8, 16):
                for T in (1, 2, 8):
                    for tw in ((), (20, 10), (32, 16), (20, 10, 7), (160,), (8, 8, 8, 8)):
                        for out in (1, 2):
                            dims = [H, *tw, out]
                            args = (d, H, E, T, len(dims) - 1, _ints(dims))
                            ok, tok = bool(lib.rs_mmoe_ok(*args)), bool(lib.rs_mmoe_train_ok(*args))
                            assert ok == expected_ok(d, H, E, T, dims), (d, H, E, T, dims)
                            assert tok == expected_train_ok(d, H, E, T, dims), (d, H, E, T, dims)
                            assert ok or not tok                      # train_ok => mmoe_ok
                            seen[tok] += 1
                            if tok:
                                assert lib.rs_mmoe_saved_size(*args, 37) == expected_saved_size(H, E, T, dims, 37)
                                assert lib.rs_mmoe_saved_size(*args, 0) == 0
                                assert lib.rs_mmoe_bwd_prepared_size(*args) == expected_bwd_prepared_size(d, H, E, T, dims)
                            else:
                                assert lib.rs_mmoe_saved_size(*args, 37) == -1
                                assert lib.rs_mmoe_bwd_prepared_size(*args) == -1
                                assert b"rs_mmoe_bwd_prepared_size" in lib.rs_last_error_string()
    assert seen[True] > 100 and seen[False] > 100
    for cfg in (TOY, TIMING):
        dims = [cfg["H"], *cfg["towers"], cfg["out"]]
        assert lib.rs_mmoe_train_ok(cfg["d"], cfg["H"], cfg["E"], cfg["T"], len(dims) - 1, _ints(dims)) == 1
    # a shape the forward takes and the backward's three tiles do not
    assert lib.rs_mmoe_ok(8, 40, 16, 8, 1, _ints([40, 1])) == 1 and lib.rs_mmoe_train_ok(8, 40, 16, 8, 1, _ints([40, 1])) == 0
    assert lib.rs_mmoe_train_ok(4, 10, 3, 3, 0, _ints([10])) == 0       # L = 0
    assert lib.rs_mmoe_train_ok(4, 10, 3, 3, 1, None) == 0
    assert lib.rs_mmoe_saved_size(4, 10, 3, 3, 3, _ints([10, 20, 10, 1]), -1) == -1


def test_abi_validation_launches_nothing_cpu():
    """Bad arguments return RS_ERR_ARG (-1) with a message before any device
    work (a launch would return RS_ERR_HIP on this device-less process, or
    fault on the fake pointers); batch 0 returns RS_OK whatever the pointers."""
    lib = _lib.lib()
    one = C.c_void_p(16)
    dims, acts = _ints([10, 20, 10, 1]), _ints([1, 1, 0])
    err = lambda: lib.rs_last_error_string()

    def fwd(x=one, prep=one, saved=one, y=one, L=3, dims=dims, acts=acts, xs=4, batch=2, E=3):
        return lib.rs_mmoe_train_fwd(x, xs, 4, 10, E, 3, L, dims, acts, prep, saved, y, 2, 1, batch, None)
    assert fwd(x=None) == -1 and b"null" in err()
    assert fwd(prep=None) == -1 and fwd(y=None) == -1
    assert fwd(saved=None) == -1 and b"saved" in err()
    assert fwd(xs=3) == -1 and b"stride" in err()
    assert fwd(L=0, dims=_ints([10])) == -1 and b"tower layers" in err()
    assert fwd(acts=_ints([3, 1, 0])) == -1 and b"activations" in err()      # sigmoid hidden layer
    assert fwd(acts=_ints([1, 1, 1])) == -1 and fwd(acts=None) == -1         # the output layer is linear
    assert fwd(E=17) == -1 and fwd(batch=-1) == -1
    assert lib.rs_mmoe_train_fwd(one, 8, 8, 40, 16, 8, 1, _ints([40, 1]), _ints([0]), one, one, one, 2, 1, 2, None) == -1
    assert fwd(x=None, prep=None, saved=None, y=None, batch=0) == 0

    def head(z=one, lab=one, G=one, zs=1, ls=1, Gs=3, T=3, nout=1, batch=2):
        return lib.rs_mmoe_head_grad(z, 2, zs, lab, 2, ls, None, nout, T, batch, G, Gs, None, None)
    assert head(z=None) == -1 and b"null" in err()
    assert head(lab=None) == -1 and head(G=None) == -1
    assert head(zs=0) == -1 and b"stride" in err()
    assert head(ls=0) == -1 and head(Gs=2) == -1 and b"G_stride" in err()
    assert head(T=0) == -1 and head(T=9) == -1 and head(nout=0) == -1 and head(batch=-1) == -1
    assert head(z=None, lab=None, G=None, batch=0) == 0

    gm, tw = (C.c_void_p * 3)(16, 16, 16), (C.c_void_p * 9)(*[16] * 9)

    def prep(em=one, g=gm, t=tw, out=one, L=3, dims=dims, E=3):
        return lib.rs_mmoe_prepare_bwd(4, 10, E, 3, em, g, L, dims, t, out, None)
    assert prep(em=None) == -1 and b"null" in err()
    assert prep(g=None) == -1 and prep(t=None) == -1 and prep(out=None) == -1
    assert prep(g=(C.c_void_p * 3)(16, None, 16)) == -1 and b"gate_matrix" in err()
    assert prep(t=(C.c_void_p * 9)(*([16] * 8 + [None]))) == -1 and b"kernel" in err()
    assert prep(L=0, dims=_ints([10])) == -1 and prep(E=0) == -1

    def bwd(saved=one, G=one, prepb=one, deltas=one, dz1=one, dx=one, Gs=3, dzs=39, dxs=4, L=3, dims=dims, acts=acts,
            batch=2):
        return lib.rs_mmoe_bwd(saved, G, Gs, 4, 10, 3, 3, L, dims, acts, prepb, deltas, dz1, dzs, dx, dxs, batch, None)
    assert bwd(saved=None) == -1 and b"null" in err()
    assert bwd(G=None) == -1 and bwd(prepb=None) == -1 and bwd(dz1=None) == -1
    assert bwd(deltas=None) == -1 and b"deltas" in err()
    assert bwd(Gs=2) == -1 and b"G_stride" in err()
    assert bwd(dzs=38) == -1 and b"dz1_stride" in err()
    assert bwd(dxs=3) == -1 and b"dx_stride" in err()
    assert bwd(L=0, dims=_ints([10])) == -1 and bwd(acts=_ints([2, 1, 0])) == -1 and bwd(batch=-1) == -1
    assert lib.rs_mmoe_bwd(one, one, 8, 8, 40, 16, 8, 1, _ints([40, 1]), _ints([0]), one, None, one, 768, None, 0, 2,
                           None) == -1
    assert bwd(saved=None, G=None, prepb=None, deltas=None, dz1=None, dx=None, batch=0) == 0


@pytest.mark.parametrize("name", sorted(CASES))
def test_mask_precondition_cpu(name):
    """Every ReLU input of the fp64 reference is away from zero, |z| > 1e-5
    rms(z) of its layer (all H E expert pre-activations and every hidden tower
    layer), so no fp32 rounding can flip a mask: the GPU comparisons below
    exclude no element."""
    c = make_case(name)
    layers = [c.ref.pre_expert] + ([np.concatenate(p, 1) for p in c.ref.pre_hidden] if c.act == "relu" else [])
    for i, z in enumerate(layers):
        assert np.abs(z).min() > 1e-5 * _rms(z), f"{name}: ReLU layer {i} has an input within 1e-5 rms of zero"


def test_gate_rule_is_about_fp32_cpu():
    """An fp32 numpy evaluation of dlogit = p (dp - sum p dp) from the
    reference's own p and dp passes gate_close — and the check is not vacuous:
    an error of 1e-4 of the terms' size fails it."""
    c = make_case("timing-B33")
    r, E, HE = c.ref, c.E, c.H * c.E
    got = []
    for t in range(c.T):
        p, dp = r.ps[t].astype(np.float32), r.dp[t].astype(np.float32)
        s = np.zeros(c.B, np.float32)
        for e in range(E):
            s = s + p[:, e] * dp[:, e]
        got.append(p * (dp - s[:, None]))
    got = np.concatenate(got, 1)
    assert got.dtype == np.float32
    gate_close(got, r.dz1[:, HE:], r.gate_terms, "fp32 numpy")
    with pytest.raises(AssertionError):
        gate_close(got + 1e-4 * _rms(r.gate_terms), r.dz1[:, HE:], r.gate_terms, "perturbed")


def test_no_cpu_training():
    import recommender_system_amd as rs
    m = rs.MMOE(10, 3, 3, [20, 10], 1, device="cpu", seed=0, input_dim=4)
    y = [np.zeros(2, np.float32)] * 3
    with pytest.raises(NotImplementedError):
        m.train_step(np.zeros((2, 4), np.float32), y)
    with pytest.raises(NotImplementedError):
        m.fit(np.zeros((2, 4), np.float32), y, epochs=1)
    assert m.train_fused_ok()
    assert not rs.MMOE(10, 3, 3, [20], 1, activation="sigmoid", device="cpu", seed=0, input_dim=4).train_fused_ok()
    assert not rs.MMOE(40, 16, 8, [], 1, device="cpu", seed=0, input_dim=8).train_fused_ok()


# --------------------------------------------------------------------- GPU
def _dev(a, gpu):
    return torch.as_tensor(np.ascontiguousarray(a)).to(gpu)


def _images(gpu, c):
    """(prepared, prepared_bwd) of case c through the raw ABI."""
    lib, st = _lib.lib(), _lib.stream()
    w = {n: _dev(v, gpu) for n, v in c.w.items()}
    p = lambda n: _lib.ptr(w.get(n))
    pa = lambda names: (C.c_void_p * len(names))(*[p(n) for n in names])
    tn = [n for t in range(c.T) for n in _tower_names(t, c.L - 1)]
    shape = (c.d, c.H, c.E, c.T)
    prep = torch.empty(lib.rs_mmoe_prepared_size(*shape, c.L, _ints(c.dims)), device=gpu)
    gms = pa([f"mmoe_layer/gate_matrix{t}" for t in range(c.T)])
    gbs = pa([f"mmoe_layer/gate_bias{t}" for t in range(c.T)]) if "mmoe_layer/gate_bias0" in w else None
    _lib.call("rs_mmoe_prepare", *shape, p("mmoe_layer/expert_matrix"), p("mmoe_layer/expert_bias"), gms, gbs, c.L,
              _ints(c.dims), pa([n + "/kernel" for n in tn]), pa([n + "/bias" for n in tn]), _lib.ptr(prep), st)
    size = lib.rs_mmoe_bwd_prepared_size(*shape, c.L, _ints(c.dims))
    assert size == expected_bwd_prepared_size(c.d, c.H, c.E, c.T, c.dims)
    prepb = torch.empty(size, device=gpu)
    _lib.call("rs_mmoe_prepare_bwd", *shape, p("mmoe_layer/expert_matrix"), gms, c.L, _ints(c.dims),
              pa([n + "/kernel" for n in tn]), _lib.ptr(prepb), st)
    torch.cuda.synchronize()  # (w may go: the images are complete)
    return prep, prepb


def _shape_args(c):
    acts = [_lib.ACT[c.act]] * (c.L - 1) + [0]
    return c.d, c.H, c.E, c.T, c.L, _ints(c.dims), _ints(acts)


def abi_train_fwd(gpu, c, prep, x):
    """(y of rs_mmoe_fwd, y of rs_mmoe_train_fwd, saved) on rows x, which live
    in a buffer c.x_pad columns wider (NaN padding)."""
    B, st = x.shape[0], _lib.stream()
    xb = torch.full((B, c.d + c.x_pad), float("nan"), device=gpu)
    xb[:, :c.d] = _dev(x, gpu)
    y0, y1 = (torch.full((c.T, B, c.out), float("nan"), device=gpu) for _ in range(2))
    _lib.call("rs_mmoe_fwd", _lib.ptr(xb), xb.stride(0), *_shape_args(c), _lib.ptr(prep), None, 0, _lib.ptr(y0),
              y0.stride(0), y0.stride(1), B, st)
    n = _lib.lib().rs_mmoe_saved_size(c.d, c.H, c.E, c.T, c.L, _ints(c.dims), B)
    assert n == expected_saved_size(c.H, c.E, c.T, c.dims, B)
    saved = torch.full((n + 8,), -7.0, device=gpu)
    _lib.call("rs_mmoe_train_fwd", _lib.ptr(xb), xb.stride(0), *_shape_args(c), _lib.ptr(prep), _lib.ptr(saved),
              _lib.ptr(y1), y1.stride(0), y1.stride(1), B, st)
    torch.cuda.synchronize()
    assert bool((saved[n:] == -7.0).all()), "saved: wrote past its size"
    return y0, y1, saved[:n]


def abi_head(gpu, c, z, labels, lw, pad=2):
    T, B, nout = z.shape
    G = torch.full((B, T * nout + pad), -7.0, device=gpu)
    loss = torch.full((T, B), float("nan"), device=gpu)
    y = _dev(labels, gpu)
    _lib.call("rs_mmoe_head_grad", _lib.ptr(z), z.stride(0), z.stride(1), _lib.ptr(y), y.stride(0), y.stride(1),
              (C.c_float * T)(*lw) if lw is not None else None, nout, T, B, _lib.ptr(G), G.stride(0), _lib.ptr(loss),
              _lib.stream())
    torch.cuda.synchronize()
    assert bool((G[:, T * nout:] == -7.0).all()), "G: wrote past T * Nout columns"
    return G, loss


def abi_bwd(gpu, c, prepb, saved, G, with_dx=True, pad=3):
    """(deltas, dz1 [B, N1], dx [B, d] or None); dz1 and dx live in wider buffers."""
    B = G.shape[0]
    nd = B * c.T * sum(c.dims[1:-1])
    deltas = torch.full((nd + 8,), -7.0, device=gpu)
    dz1 = torch.full((B, c.N1 + pad), -7.0, device=gpu)
    dx = torch.full((B, c.d + pad), -7.0, device=gpu) if with_dx else None
    _lib.call("rs_mmoe_bwd", _lib.ptr(saved), _lib.ptr(G), G.stride(0), *_shape_args(c), _lib.ptr(prepb),
              _lib.ptr(deltas), _lib.ptr(dz1), dz1.stride(0), _lib.ptr(dx), dx.stride(0) if with_dx else 0, B,
              _lib.stream())
    torch.cuda.synchronize()
    assert bool((deltas[nd:] == -7.0).all()) and bool((dz1[:, c.N1:] == -7.0).all())
    assert not with_dx or bool((dx[:, c.d:] == -7.0).all())
    return deltas[:nd], dz1[:, :c.N1].contiguous(), dx[:, :c.d].contiguous() if with_dx else None


class Run:
    pass


@functools.lru_cache(maxsize=None)
def run_case(name):
    """Every kernel of the step on case `name`, once; shared (never modified)
    by the tests below."""
    gpu = torch.device("cuda")
    c = make_case(name)
    r = Run()
    r.prep, r.prepb = _images(gpu, c)
    r.y0, r.y1, r.saved = abi_train_fwd(gpu, c, r.prep, c.x)
    r.G, r.loss = abi_head(gpu, c, r.y1, c.labels, c.lw)
    r.deltas, r.dz1, r.dx = abi_bwd(gpu, c, r.prepb, r.saved, r.G)
    return r


def saved_blocks(c, saved, B):
    """saved (or, with its first three blocks dropped, deltas) as arrays."""
    out, o = [], 0
    for wd in [c.H * c.E, c.T * c.E, c.T * c.H] + [c.T * n for n in c.dims[1:-1]]:
        out.append(saved[o:o + B * wd].view(B, wd))
        o += B * wd
    assert o == saved.numel()
    return out


def delta_blocks(c, deltas, B):
    out, o = [], 0
    for n in c.dims[1:-1]:
        out.append(deltas[o:o + B * c.T * n].view(B, c.T * n))
        o += B * c.T * n
    return out


@gpu_test
@pytest.mark.parametrize("name", sorted(CASES))
def test_train_fwd(gpu, name):
    c, r = make_case(name), run_case(name)
    assert bool(torch.isfinite(r.y0).all()) and torch.equal(r.y1, r.y0), "y differs from rs_mmoe_fwd's"
    for t in range(c.T):
        assert_scaled_close(r.y1[t], c.ref.z[t], what=f"{name}: tower {t}")
    blocks = saved_blocks(c, r.saved, c.B)
    for got, ref, what in zip(blocks, [c.ref.expert, c.ref.gates, c.ref.mix] + c.ref.a,
                              ["expert", "gates", "mix"] + [f"a_{l}" for l in range(c.L - 1)]):
        assert_scaled_close(got, ref, what=f"{name}: saved {what}")
    if c.E == 1:
        assert bool((blocks[1] == 1.0).all()) and torch.equal(blocks[2][:, :c.H], blocks[0])


@gpu_test
@pytest.mark.parametrize("name", sorted(CASES))
def test_head_grad(gpu, name):
    c, r = make_case(name), run_case(name)
    assert_scaled_close(r.G[:, :c.T * c.out], c.ref.G, what=f"{name}: G")
    assert_scaled_close(r.loss, c.ref.loss, what=f"{name}: loss")
    # loss_weights NULL = all ones; loss NULL is allowed
    z = r.y1
    G1, _ = abi_head(gpu, c, z, c.labels, None)
    G2, _ = abi_head(gpu, c, z, c.labels, [1.0] * c.T)
    assert torch.equal(G1, G2)


@gpu_test
@pytest.mark.parametrize("name", sorted(CASES))
def test_bwd(gpu, name):
    c, r = make_case(name), run_case(name)
    HE = c.H * c.E
    for l, (got, ref) in enumerate(zip(delta_blocks(c, r.deltas, c.B), c.ref.deltas)):
        assert_scaled_close(got, ref, what=f"{name}: delta_{l}")
    assert_scaled_close(r.dz1[:, :HE], c.ref.dz1[:, :HE], what=f"{name}: dz1, experts")
    gate_close(r.dz1[:, HE:].cpu().numpy(), c.ref.dz1[:, HE:], c.ref.gate_terms, f"{name}: dz1, gates")
    assert_scaled_close(r.dx, c.ref.dx, what=f"{name}: dx")
    if c.E == 1:
        assert bool((r.dz1[:, HE:] == 0).all())  # p = 1: dp - p dp, exactly


@gpu_test
@pytest.mark.parametrize("name", ["toy-B33", "timing-B33", "kslices"])
def test_contracts_bit_exact(gpu, name):
    c, r = make_case(name), run_case(name)
    B = c.B
    # run to run
    y0, y1, saved = abi_train_fwd(gpu, c, r.prep, c.x)
    assert torch.equal(y1, r.y1) and torch.equal(saved, r.saved)
    deltas, dz1, dx = abi_bwd(gpu, c, r.prepb, r.saved, r.G)
    assert torch.equal(deltas, r.deltas) and torch.equal(dz1, r.dz1) and torch.equal(dx, r.dx)
    # dz1 and the deltas with dx NULL
    deltas, dz1, none = abi_bwd(gpu, c, r.prepb, r.saved, r.G, with_dx=False)
    assert none is None and torch.equal(deltas, r.deltas) and torch.equal(dz1, r.dz1)
    # rows in a batch of one tile fewer / at another place in their tile: the forward from x, the backward from
    # the same rows of saved and G (G itself carries the batch size, 1 / (B Nout))
    full_s, full_d = saved_blocks(c, r.saved, B), delta_blocks(c, r.deltas, B)
    for rows in (slice(0, B - 16), slice(min(17, B - 2), min(25, B)), slice(B - 1, B)):
        n = len(range(*rows.indices(B)))
        _, y_sub, saved_sub = abi_train_fwd(gpu, c, r.prep, c.x[rows])
        assert torch.equal(y_sub, r.y1[:, rows])
        want = torch.cat([b[rows].reshape(-1) for b in full_s])
        assert torch.equal(saved_sub, want)
        d_sub, dz_sub, dx_sub = abi_bwd(gpu, c, r.prepb, want, r.G[rows].contiguous())
        assert torch.equal(dz_sub, r.dz1[rows]) and torch.equal(dx_sub, r.dx[rows])
        for got, full in zip(delta_blocks(c, d_sub, n), full_d):
            assert torch.equal(got, full[rows])


def _model(gpu, c):
    import recommender_system_amd as rs
    m = rs.MMOE(c.H, c.E, c.T, list(c.towers), c.out, activation=c.act,
                use_expert_bias="mmoe_layer/expert_bias" in c.w, use_gate_bias="mmoe_layer/gate_bias0" in c.w,
                device=gpu, seed=0, input_dim=c.d)
    m.set_keras_weights(c.w)
    return m


def _weights_close(m, ref, what, rtol=RTOL):
    got = m.keras_weights()
    assert set(got) == set(ref)
    for k, v in ref.items():
        assert_scaled_close(got[k], v, rtol=rtol, what=f"{what}: {k}")


@gpu_test
@pytest.mark.parametrize("name", ["toy-B33", "timing-B33", "nobias", "linear", "L1", "Nout2", "kslices"])
def test_gradients(gpu, name):
    c = make_case(name)
    m = _model(gpu, c)
    assert m.train_fused_ok()
    before = {k: v.clone() for k, v in m.keras_weights().items()}
    gf, lf, dxf = m.gradients(c.x, list(c.labels), c.lw, fused=True, want_dx=True)
    gc, lc, dxc = m.gradients(c.x, torch.as_tensor(c.labels), c.lw, fused=False, want_dx=True)
    ga, _, none = m.gradients(c.x, c.labels, c.lw)
    assert none is None and set(gf) == set(c.ref.grads) == set(gc) == set(m.keras_weights())
    for k, ref in c.ref.grads.items():
        assert tuple(gf[k].shape) == tuple(m.keras_weights()[k].shape) and gf[k].is_contiguous()
        assert_scaled_close(gf[k], ref, what=f"{name}: fused d {k}")
        assert_scaled_close(gc[k], ref, what=f"{name}: composed d {k}")
        assert_scaled_close(gf[k], gc[k].cpu().numpy(), what=f"{name}: fused vs composed d {k}")
        assert torch.equal(ga[k], gf[k])                     # fused=None picks the kernels
    for got in (lf, lc):
        assert_scaled_close(got, c.ref.loss, what=f"{name}: losses")
    for got in (dxf, dxc):
        assert_scaled_close(got, c.ref.dx, what=f"{name}: dx")
    assert all(torch.equal(v, before[k]) for k, v in m.keras_weights().items())   # gradients() updates nothing


@gpu_test
@pytest.mark.parametrize("name,fused", [("toy-B33", True), ("toy-B33", False), ("nobias", True), ("Nout2", None)])
def test_train_step(gpu, name, fused):
    c = make_case(name)
    m = _model(gpu, c)
    loss = m.train_step(c.x, list(c.labels), lr=0.01, loss_weights=c.lw, return_loss=True, fused=fused)
    assert_scaled_close(loss, c.ref.loss, what=f"{name}: return_loss")
    _weights_close(m, c.ref.new, f"{name}: after 1 step")
    w = c.ref.new
    for _ in range(2):
        w = mmoe_train_ref(c.x, c.labels, w, 0.01, c.lw, c.act).new
        ret = m.train_step(c.x, c.labels, lr=0.01, loss_weights=c.lw, fused=fused)
        assert ret is None
    _weights_close(m, w, f"{name}: after 3 steps")
    # the forward sees the new weights (both images were dropped)
    y = m(c.x)
    ref = mmoe_train_ref(c.x, c.labels, w, 0.01, c.lw, c.act)
    for t in range(c.T):
        assert_scaled_close(y[t], ref.z[t], what=f"{name}: forward after the steps, tower {t}")
    loss, dx = m.train_step(c.x, c.labels, lr=0.01, loss_weights=c.lw, return_loss=True, return_dx=True, fused=fused)
    assert_scaled_close(loss, ref.loss, what=f"{name}: loss of step 4")
    assert_scaled_close(dx, ref.dx, what=f"{name}: dx of step 4")


@gpu_test
@pytest.mark.parametrize("fused", [True, False])
def test_l2_pull_alone(gpu, fused):
    """loss_weights 0 makes G exactly 0: every gradient is 0, so the towers do
    not move at all and each mmoe_layer tensor moves by lr * 2e-4 * w (one
    fp32 rounding of the product or of the fused multiply-add: within one ulp
    of w)."""
    c = make_case("toy-B19")
    m = _model(gpu, c)
    m.train_step(c.x, c.labels, lr=0.5, loss_weights=[0.0] * c.T, fused=fused)
    moved = 0
    for k, v in m.keras_weights().items():
        got, w0 = v.cpu().numpy(), c.w[k]
        if k.startswith(MMOE_LAYER):
            want = w0.astype(np.float64) * (1 - 0.5 * 2e-4)
            assert (np.abs(got - want) <= np.spacing(np.abs(w0))).all(), k
            moved += int((got != w0).sum())
        else:
            assert np.array_equal(got, w0), k
    assert moved > 100


@gpu_test
def test_refused_shape_and_bad_arguments(gpu):
    import recommender_system_amd as rs
    rng = np.random.default_rng(3)
    m = rs.MMOE(40, 16, 8, [], 1, device=gpu, seed=0, input_dim=8)     # the backward's tiles do not fit
    x = rng.normal(size=(5, 8)).astype(np.float32)
    y = rng.integers(0, 2, (8, 5)).astype(np.float32)
    assert m.fused_ok() and not m.train_fused_ok()
    with pytest.raises(ValueError, match="fused=True"):
        m.train_step(x, y, fused=True)
    w0 = {k: v.cpu().numpy().copy() for k, v in m.keras_weights().items()}
    loss = m.train_step(x, y, return_loss=True)                        # None: the composition
    ref = mmoe_train_ref(x, y.reshape(8, 5, 1), w0, 0.01)
    assert_scaled_close(loss, ref.loss, what="refused shape: losses")
    _weights_close(m, ref.new, "refused shape")
    with pytest.raises(NotImplementedError):
        rs.MMOE(10, 3, 3, [20], 1, activation="sigmoid", device=gpu, seed=0, input_dim=4).train_step(
            np.zeros((2, 4), np.float32), np.zeros((3, 2), np.float32))
    c = make_case("toy-B19")
    with pytest.raises(ValueError):
        _model(gpu, c).train_step(c.x, list(c.labels)[:2])
    with pytest.raises(ValueError):
        _model(gpu, c).train_step(c.x, c.labels, loss_weights=[1.0])


@gpu_test
def test_fit(gpu):
    """Two epochs over 70 rows at batch 32: batches of 32, 32 and 6."""
    c = make_case("toy-B19")
    rng = np.random.default_rng(11)
    x = rng.normal(0, 1, (70, c.d)).astype(np.float32)
    labels = rng.integers(0, 2, (c.T, 70, 1)).astype(np.float32)
    m = _model(gpu, c)
    hist = m.fit(x, [labels[t, :, 0] for t in range(c.T)], batch_size=32, epochs=2, lr=0.05, loss_weights=c.lw)
    want, w = fit_ref(x, labels, c.w, 32, 2, 0.05, c.lw)
    assert len(hist) == 2 and want[1] < want[0]
    np.testing.assert_allclose(hist, want, rtol=RTOL)
    _weights_close(m, w, "fit")
