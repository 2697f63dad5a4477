"""The kernels the training steps are composed from, one by one, against plain
numpy float64 restatements of the formulas in include/rs_capi.h.

Part A (CPU): every backward reference is pinned by central finite
differences of its forward reference (a random linear functional of the
output, step 1e-6, agreement 1e-6), and the argument checks that reject a
shape before any device work are called with dummy pointers.

Part B (GPU): each kernel at the shapes where it changes path (lane groups
against lane-per-column, one block per sample against the generic kernel, a
row that is no multiple of the wave, the LDS and register limits), with row
strides wider than the row (NaN in the input padding, a sentinel in the
output padding), accumulated outputs prefilled with random values and stored
ones with NaN, every optional pointer present and absent, and run twice for
bitwise equality.

Tolerances: element-wise outputs and sums over at most a row: the project's
contract (helpers.assert_scaled_close at 1e-5).  Sums over the batch and
differences of such sums: |err| <= 2e-6 * sum |terms| (the bound of
test_rs_gemm_mfma_matches_torch), sum |terms| from the reference run on
absolute values.
"""
import ctypes as C

import numpy as np
import pytest

from oracle import ctr_oracle as O
from recommender_system_amd import _lib
from tests.helpers import RTOL, assert_scaled_close

torch = pytest.importorskip("torch")

SUM_TOL = 2e-6  # per sum |terms| (tests/test_train.py::test_rs_gemm_mfma_matches_torch)
F64 = np.float64
F32 = np.float32


def _d(a):
    return np.asarray(a, F64)


# --------------------------------------------------------------------------
# References (float64).  `ab=True` runs the same sums on absolute values: the
# sum |terms| of every output, for the bound of the batch sums.
# --------------------------------------------------------------------------
def ref_bn_stats(x):
    x = _d(x)
    return x.mean(0), x.var(0)


def ref_bn_apply(x, mean, var, gamma, beta, eps):
    return (_d(x) - _d(mean)) / np.sqrt(_d(var) + eps) * _d(gamma) + _d(beta)


def ref_bn_bwd(x, mean, var, gamma, eps, dy, ab=False):
    """rs_bn_train_bwd from the saved batch statistics."""
    x, dy, gamma = _d(x), _d(dy), _d(gamma)
    B = x.shape[0]
    inv = 1.0 / np.sqrt(_d(var) + eps)
    xh = (x - _d(mean)) * inv
    if ab:
        xh, dy, gamma = np.abs(xh), np.abs(dy), np.abs(gamma)
    dbeta, dgamma = dy.sum(0), (dy * xh).sum(0)
    sgn = 1.0 if ab else -1.0
    dx = gamma * inv * (dy + sgn * dbeta / B + sgn * xh * dgamma / B)
    return dx, dgamma, dbeta


def ref_pool(score, live, seq):
    """rs_masked_softmax_pool: score [B,T], live [B,T] bool, seq [B,T,K]."""
    s = np.where(live, _d(score), -2.0 ** 32)  # -2**32 + 1 rounds to -2**32 in fp32
    e = np.exp(s - s.max(1, keepdims=True))
    a = e / e.sum(1, keepdims=True)
    return a, np.einsum("bt,btk->bk", a, _d(seq))


def ref_pool_bwd(a, live, seq, datt):
    a, seq, datt = _d(a), _d(seq), _d(datt)
    da = np.einsum("bk,btk->bt", datt, seq)
    dot = (a * da).sum(1, keepdims=True)
    return np.where(live, a * (da - dot), 0.0), a[:, :, None] * datt[:, None, :]


def ref_concat(q, s):
    """rs_din_att_concat: q [B,K], s [B,T,K] -> [B,T,4K]."""
    q, s = _d(q), _d(s)
    qb = np.broadcast_to(q[:, None, :], s.shape)
    return np.concatenate([qb, s, qb - s, qb * s], -1)


def ref_concat_bwd(d, q, s):
    d, q, s = _d(d), _d(q), _d(s)
    K = q.shape[1]
    d0, d1, d2, d3 = (d[..., i * K:(i + 1) * K] for i in range(4))
    return (d0 + d2 + s * d3).sum(1), d1 - d2 + q[:, None, :] * d3


def _alpha_rows(alpha, M, N, period):
    return _d(alpha).reshape(period, N)[np.arange(M) % period]


def ref_prelu_rows(z, alpha, period):
    z = _d(z)
    return O.prelu(z, _alpha_rows(alpha, z.shape[0], z.shape[1], period))


def ref_prelu_rows_bwd(z, dy, alpha, period, ab=False):
    """dz = dy (z > 0 ? 1 : alpha), dalpha[p, c] = sum_{r = p mod period} dy min(z, 0)."""
    z, dy = _d(z), _d(dy)
    M, N = z.shape
    al = _alpha_rows(alpha, M, N, period)
    neg = np.minimum(z, 0.0)
    if ab:
        al, neg = np.abs(al), np.abs(neg)
    dz = dy * np.where(z > 0, 1.0, al)
    return dz, (dy * neg).reshape(M // period, period, N).sum(0)


def ref_att_fwd(h0, W1, b1, al1, W2, b2, al2, wo, bo, T):
    """rs_din_att_prelu_fwd: h0 [B*T, K0] -> z1, z2, score."""
    z1 = _d(h0) @ _d(W1) + _d(b1)
    z2 = ref_prelu_rows(z1, al1, T) @ _d(W2) + _d(b2)
    return z1, z2, ref_prelu_rows(z2, al2, T) @ _d(wo).reshape(-1) + float(np.asarray(bo).reshape(-1)[0])


def ref_att_bwd(h0, z1, z2, ds, W1, W2, al1, al2, wo, T, ab=False):
    """rs_din_att_prelu_bwd: dh0, dW1, db1, dalpha1, dW2, db2, dalpha2, dwo, dbo."""
    f = np.abs if ab else (lambda v: v)
    h0, ds, W1, W2, wo = f(_d(h0)), f(_d(ds)), f(_d(W1)), f(_d(W2)), f(_d(wo).reshape(-1))
    y1, y2 = f(ref_prelu_rows(z1, al1, T)), f(ref_prelu_rows(z2, al2, T))
    dwo, dbo = y2.T @ ds, ds.sum(keepdims=True)
    dz2, dal2 = ref_prelu_rows_bwd(z2, ds[:, None] * wo[None, :], al2, T, ab)
    dW2, db2 = y1.T @ dz2, dz2.sum(0)
    dz1, dal1 = ref_prelu_rows_bwd(z1, dz2 @ W2.T, al1, T, ab)
    return dz1 @ W1.T, h0.T @ dz1, dz1.sum(0), dal1, dW2, db2, dal2, dwo, dbo


ATT_NAMES = ("dh0", "dW1", "db1", "dalpha1", "dW2", "db2", "dalpha2", "dwo", "dbo")


def ref_cross_fwd(x0, W, b):
    """rs_cross_train_fwd: xs [L,B,d] (x_1..x_L), g [L,B], x_L."""
    x0, W, b = _d(x0), _d(W), _d(b)
    x, xs, g = x0, [], []
    for l in range(W.shape[0]):
        g.append(x @ W[l])
        x = x0 * g[-1][:, None] + b[l] + x
        xs.append(x)
    B, d = x0.shape
    return np.array(xs).reshape(len(xs), B, d), np.array(g).reshape(len(g), B), x


def ref_cross_bwd(x0, W, g, dxl):
    """rs_cross_train_bwd: deltas [L,B,d], s [L,B] and the addend of dx."""
    x0, W, g, delta = _d(x0), _d(W), _d(g), _d(dxl)
    L = W.shape[0]
    deltas, s, acc = [None] * L, [None] * L, np.zeros_like(x0)
    for l in range(L - 1, -1, -1):
        deltas[l] = delta
        s[l] = (x0 * delta).sum(1)
        acc = acc + g[l][:, None] * delta
        delta = delta + s[l][:, None] * W[l]
    B, d = x0.shape
    return np.array(deltas).reshape(L, B, d), np.array(s).reshape(L, B), delta + acc


def ref_inner_bwd(e, dinner, dflat):
    """rs_inner_product_bwd: e, dflat [B,F,k], dinner [B,P]."""
    e, dinner = _d(e), _d(dinner)
    row, col = O.pair_indices(e.shape[1])
    de = _d(dflat).copy()
    for p, (i, j) in enumerate(zip(row, col)):
        de[:, i] += dinner[:, p, None] * e[:, j]
        de[:, j] += dinner[:, p, None] * e[:, i]
    return de


def ref_bi_bwd(e, dbi):
    e = _d(e)
    return _d(dbi)[:, None, :] * (e.sum(1, keepdims=True) - e)


def ref_bce_prob(pre, t):
    """rs_bce_prob_grad: per-sample loss (O.pnn_bce) and g = dL/dpre."""
    pre, t = _d(pre).reshape(-1), _d(t).reshape(-1)
    eps, ybar = O.KERAS_EPS, t.mean()
    q = np.clip(pre, eps, 1 - eps)
    inside = (pre >= eps) & (pre <= 1 - eps)
    g = np.where(inside, (-ybar / (q + eps) + (1 - ybar) / (1 - q + eps)) / pre.size, 0.0)
    return g, O.pnn_bce(pre, t)[1]


def ref_head(fm, dnn, t, c_fm, c_dnn):
    z = c_fm * _d(fm) + c_dnn * _d(dnn)
    g = (O.sigmoid(z) - _d(t)) / z.size
    return c_fm * g, c_dnn * g, np.maximum(z, 0) - z * _d(t) + np.log1p(np.exp(-np.abs(z)))


def ref_ffm_train(dense, ids, vocab, w0, w, v, t):
    """rs_ffm_train_fwd: G [B, NF*k], g [B], loss [B]; z from O.ffm_layer_gather."""
    dense, v, t = _d(dense), _d(v), _d(t)
    B, nd = dense.shape
    ids = np.asarray(ids).astype(np.int64)
    offs = np.concatenate([[0], np.cumsum(vocab)[:-1]]).astype(np.int64)
    ok = (ids >= 0) & (ids < np.asarray(vocab)[None, :])
    rows = np.where(ok, nd + offs[None, :] + ids, 0)
    Fm = np.einsum("bi,ifk->bfk", dense, v[:nd]) + np.einsum("bc,bcfk->bfk", ok.astype(F64), v[rows])
    z = O.ffm_layer_gather(dense, ids, vocab, _d(w0), _d(w), v)[:, 0]
    g = (O.sigmoid(z) - t) / B
    G = g[:, None, None] * (Fm.sum(1, keepdims=True) - Fm)
    return G.reshape(B, -1), g, np.maximum(z, 0) - z * t + np.log1p(np.exp(-np.abs(z))), z


def ref_fm_grads(x, s, w1, v, g, ab=False):
    """rs_fm_x_grad's addend and rs_fm_param_grads' dw1, dv, dw0."""
    f = np.abs if ab else (lambda a: a)
    x, s, w1, v, g = f(_d(x)), f(_d(s)), f(_d(w1)), f(_d(v)), f(_d(g))
    sgn = 1.0 if ab else -1.0
    dx = g[:, None] * (w1[None, :] + s @ v.T + sgn * x * (v * v).sum(1)[None, :])
    gx = g[:, None] * x
    dv = gx.T @ s + sgn * (gx * x).sum(0)[:, None] * v
    return dx, gx.sum(0), dv, g.sum(keepdims=True)


# --------------------------------------------------------------------------
# A. CPU: finite differences pin every backward reference
# --------------------------------------------------------------------------
def _fd(f, x, h=1e-6):
    """Central differences of the scalar f() with respect to the array x (in place)."""
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


def test_fd_bn():
    rng = np.random.default_rng(1)
    B, D, eps = 7, 3, 1e-3
    x, gamma, beta = rng.normal(size=(B, D)), rng.normal(size=D), rng.normal(size=D)
    c = rng.normal(size=(B, D))

    def f():
        mean, var = ref_bn_stats(x)
        return float((c * ref_bn_apply(x, mean, var, gamma, beta, eps)).sum())

    mean, var = ref_bn_stats(x)
    dx, dgamma, dbeta = ref_bn_bwd(x, mean, var, gamma, eps, c)
    _fd_close(_fd(f, x), dx, "bn dx")
    _fd_close(_fd(f, gamma), dgamma, "bn dgamma")
    _fd_close(_fd(f, beta), dbeta, "bn dbeta")


def test_fd_masked_softmax_pool():
    rng = np.random.default_rng(2)
    B, T, K = 4, 6, 3
    score, seq = 3 * rng.normal(size=(B, T)), rng.normal(size=(B, T, K))
    live = rng.random((B, T)) < 0.6
    live[0] = False  # fully padded: a = 1/T, no gradient to the score
    live[1] = False
    live[1, 2] = True
    live[2] = True
    c = rng.normal(size=(B, K))
    f = lambda: float((c * ref_pool(score, live, seq)[1]).sum())
    a, _ = ref_pool(score, live, seq)
    np.testing.assert_allclose(a[0], 1.0 / T, rtol=1e-15)
    assert np.all(a[1][~live[1]] == 0.0) and a[1, 2] == 1.0
    ds, dseq = ref_pool_bwd(a, live, seq, c)
    assert np.all(ds[0] == 0.0)
    _fd_close(_fd(f, score), ds, "pool ds")
    _fd_close(_fd(f, seq), dseq, "pool dseq")


def test_fd_att_concat():
    rng = np.random.default_rng(3)
    B, T, K = 2, 3, 4
    q, s, c = rng.normal(size=(B, K)), rng.normal(size=(B, T, K)), rng.normal(size=(B, T, 4 * K))
    f = lambda: float((c * ref_concat(q, s)).sum())
    dq, dseq = ref_concat_bwd(c, q, s)
    _fd_close(_fd(f, q), dq, "concat dq")
    _fd_close(_fd(f, s), dseq, "concat dseq")


def test_fd_prelu_rows_with_period():
    rng = np.random.default_rng(4)
    period, N = 3, 4
    M = 2 * period
    z, alpha, c = rng.normal(size=(M, N)), rng.normal(size=(period, N)), rng.normal(size=(M, N))
    assert np.abs(z).min() > 1e-4  # away from the kink
    f = lambda: float((c * ref_prelu_rows(z, alpha, period)).sum())
    dz, dalpha = ref_prelu_rows_bwd(z, c, alpha, period)
    _fd_close(_fd(f, z), dz, "prelu dz")
    _fd_close(_fd(f, alpha), dalpha, "prelu dalpha")


def test_fd_att_prelu_unit():
    rng = np.random.default_rng(5)
    B, T, K0, h1, h2 = 2, 3, 4, 5, 3
    M = B * T
    h0 = rng.normal(size=(M, K0))
    W1, b1, al1 = rng.normal(size=(K0, h1)), rng.normal(size=h1), rng.normal(size=(T, h1))
    W2, b2, al2 = rng.normal(size=(h1, h2)), rng.normal(size=h2), rng.normal(size=(T, h2))
    wo, bo, c = rng.normal(size=h2), rng.normal(size=1), rng.normal(size=M)
    fwd = lambda: ref_att_fwd(h0, W1, b1, al1, W2, b2, al2, wo, bo, T)
    f = lambda: float((c * fwd()[2]).sum())
    z1, z2, _ = fwd()
    assert min(np.abs(z1).min(), np.abs(z2).min()) > 1e-4
    grads = ref_att_bwd(h0, z1, z2, c, W1, W2, al1, al2, wo, T)
    for name, arr, g in zip(ATT_NAMES, (h0, W1, b1, al1, W2, b2, al2, wo, bo), grads):
        _fd_close(_fd(f, arr), g.reshape(arr.shape), "att unit " + name)


def test_fd_crossnet():
    rng = np.random.default_rng(6)
    B, d, L = 3, 5, 3
    x0, W, b = rng.normal(size=(B, d)), rng.normal(size=(L, d)) / np.sqrt(d), rng.normal(size=(L, d))
    c = rng.normal(size=(B, d))
    f = lambda: float((c * ref_cross_fwd(x0, W, b)[2]).sum())
    xs, g, _ = ref_cross_fwd(x0, W, b)
    deltas, s, dx = ref_cross_bwd(x0, W, g, c)
    _fd_close(_fd(f, x0), dx, "cross dx0")
    xl = np.concatenate([x0[None], xs[:-1]])  # x_0 .. x_{L-1}
    _fd_close(_fd(f, W), np.einsum("lb,lbd->ld", s, xl), "cross dW (from s)")
    _fd_close(_fd(f, b), deltas.sum(1), "cross db (from deltas)")
    assert np.array_equal(ref_cross_bwd(x0, W[:0], g[:0], c)[2], c)  # L = 0: dx += dxl


def test_fd_inner_product_and_bi_interaction():
    rng = np.random.default_rng(7)
    B, F, k = 2, 4, 3
    e = rng.normal(size=(B, F, k))
    cf, ci, cb = rng.normal(size=(B, F, k)), rng.normal(size=(B, F * (F - 1) // 2)), rng.normal(size=(B, k))
    f = lambda: float((cf * e).sum() + (ci * O.inner_product_layer(e)).sum())
    _fd_close(_fd(f, e), ref_inner_bwd(e, ci, cf), "inner product demb")
    fb = lambda: float((cb * O.bi_interaction(e)).sum())
    _fd_close(_fd(fb, e), ref_bi_bwd(e, cb), "bi-interaction demb")


def test_fd_losses_and_fm():
    rng = np.random.default_rng(8)
    B, d, kfm = 5, 4, 3
    pre, t = rng.uniform(0.05, 0.95, B), rng.integers(0, 2, B).astype(F64)
    g, per = ref_bce_prob(pre, t)
    _fd_close(_fd(lambda: float(O.pnn_bce(pre, t)[0]), pre), g, "bce prob g")
    fm, dnn = rng.normal(size=B), rng.normal(size=B)
    g_fm, g_dnn, _ = ref_head(fm, dnn, t, 0.5, 0.25)
    fh = lambda: float(ref_head(fm, dnn, t, 0.5, 0.25)[2].mean())
    _fd_close(_fd(fh, fm), g_fm, "head g_fm")
    _fd_close(_fd(fh, dnn), g_dnn, "head g_dnn")
    x, w0, w1, v, c = rng.normal(size=(B, d)), rng.normal(size=1), rng.normal(size=d), rng.normal(size=(d, kfm)), \
        rng.normal(size=B)
    ffm = lambda: float((c * O.fm_layer(x, w0, w1.reshape(-1, 1), v)[:, 0]).sum())
    dx, dw1, dv, dw0 = ref_fm_grads(x, x @ v, w1, v, c)
    for arr, gr, name in ((x, dx, "dx"), (w1, dw1, "dw1"), (v, dv, "dv"), (w0, dw0, "dw0")):
        _fd_close(_fd(ffm, arr), gr, "fm " + name)


# --------------------------------------------------------------------------
# A. CPU: shapes past a kernel's limit are refused before any device work
# --------------------------------------------------------------------------
def _p(i):
    return C.c_void_p(0x1000 * i)  # distinct dummy non-null pointers; nothing launches


def _refused(status, *words):
    msg = _lib.lib().rs_last_error_string()
    assert status == -1, (status, msg)
    for w in words:
        assert w in msg, msg


def test_limits_refused_without_device():
    lib = _lib.lib()
    _refused(lib.rs_cross_train_fwd(_p(1), 2049, 2049, 1, _p(2), _p(3), 4, _p(4), _p(5), None, 0, None),
             b"rs_cross_train_fwd", b"d <= 2048")
    _refused(lib.rs_cross_train_bwd(_p(1), 2049, 2049, 1, _p(2), 4, _p(3), _p(4), 2049, _p(5), _p(6), _p(7), 2049,
                                    None), b"rs_cross_train_bwd", b"d <= 2048")
    _refused(lib.rs_masked_softmax_pool(_p(1), _p(2), _lib.ID_I32, 513, _p(3), 4, 513, 8, _p(4), _p(5), 8, None),
             b"rs_masked_softmax_pool:", b"T <= 512")
    _refused(lib.rs_masked_softmax_pool_bwd(_p(1), _p(2), _lib.ID_I32, 513, _p(3), _p(4), 8, 4, 513, 8, _p(5), _p(6),
                                            None), b"rs_masked_softmax_pool_bwd", b"T <= 512")
    for F, k in ((65, 4), (4, 65)):
        P = F * (F - 1) // 2
        _refused(lib.rs_inner_product_bwd(_p(1), F * k, _p(2), P, _p(3), F * k, F, k, 4, _p(4), F * k, None),
                 b"rs_inner_product_bwd", b"n_fields <= 64, k <= 64")
    _refused(lib.rs_prelu_rows_bwd(_p(1), _p(2), 10, 4, _p(3), 3, _p(4), _p(5), _p(6), 1 << 20, None),
             b"rs_prelu_rows_bwd", b"multiple of period")
    _refused(lib.rs_bn_train_bwd(_p(1), 4, 8, 4, _p(2), _p(3), _p(4), 1e-3, _p(5), 4, _p(5), 4, _p(6), _p(7), None),
             b"rs_bn_train_bwd")
    _refused(lib.rs_din_att_prelu_fwd(*[_p(i) for i in range(1, 10)], 4, 8, 30, 80, 40, _p(10), _p(11), _p(12), None),
             b"rs_din_att_prelu_fwd", b"unsupported shape")


ATT_OK = [(100, 32, 80, 40), (30, 64, 80, 40), (64, 128, 64, 64), (128, 64, 64, 32), (64, 128, 80, 40),
          (17, 12, 20, 12), (1, 4, 4, 4)]
ATT_REFUSED = [(64, 128, 128, 128), (128, 64, 64, 64), (128, 128, 80, 40), (30, 30, 80, 40), (129, 32, 80, 40),
               (20, 132, 80, 40)]


def test_att_unit_workspace_size_table():
    size = _lib.lib().rs_din_att_prelu_bwd_workspace_size
    for T, K0, h1, h2 in ATT_OK:
        assert size(4, T, K0, h1, h2) > 0, (T, K0, h1, h2)
    for T, K0, h1, h2 in ATT_REFUSED:
        assert size(4, T, K0, h1, h2) == -1, (T, K0, h1, h2)
    # G = min(B, 256) workgroups, one partial of every parameter gradient each
    T, K0, h1, h2 = 17, 12, 20, 12
    P = K0 * h1 + h1 * h2 + T * h1 + T * h2 + h1 + h2 + h2 + 1
    assert size(4, T, K0, h1, h2) == 4 * P * 4 and size(300, T, K0, h1, h2) == 256 * P * 4


# --------------------------------------------------------------------------
# B. GPU
# --------------------------------------------------------------------------
SENT = -12345.75  # output padding: must come back untouched
WORST = {}        # kernel -> [worst scaled error, worst error / sum |terms|]


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    yield
    for k in sorted(WORST):
        print(f"\nworst {k}: scaled {WORST[k][0]:.3e}  batch sums / sum|terms| {WORST[k][1]:.3e}", end="")


def _dev(a, dtype=F32):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype))).to("cuda")


def _rows(a, pad=0, fill=np.nan, dtype=F32):
    """[R, W] on the device with row stride W + pad; the padding holds `fill`."""
    a = np.asarray(a, dtype)
    buf = np.full((a.shape[0], a.shape[1] + pad), fill, dtype)
    buf[:, :a.shape[1]] = a
    return _dev(buf, dtype)


def _out(R, W, pad=0, old=None):
    """An output [R, W]: NaN (stored) or `old` (accumulated), sentinel padding."""
    return _rows(np.full((R, W), np.nan, F32) if old is None else old, pad, SENT)


def _get(t, W=None):
    a = t.detach().cpu().numpy()
    if W is not None:
        assert np.all(a[:, W:] == SENT), "a kernel wrote into the padding of a strided output"
        a = a[:, :W]
    return a


def _nrm(rng, *shape):
    return rng.standard_normal(shape).astype(F32)


def _close(kernel, got, ref, what, rtol=RTOL):
    got, ref = np.asarray(_get(got) if hasattr(got, "detach") else got, F64).reshape(np.shape(ref)), _d(ref)
    if ref.size:
        scale = np.maximum(np.abs(ref), float(np.sqrt(np.mean(ref ** 2)))) + 1e-300
        w = WORST.setdefault(kernel, [0.0, 0.0])
        w[0] = max(w[0], float(np.nanmax(np.abs(got - ref) / scale)))
    assert_scaled_close(got, ref, rtol, f"{kernel} {what}")


def _sum_close(kernel, got, ref, absum, what, factor=SUM_TOL, extra=0.0):
    """|got - ref| <= factor * sum |terms| (+ extra)."""
    got, ref = np.asarray(_get(got) if hasattr(got, "detach") else got, F64).reshape(np.shape(ref)), _d(ref)
    absum = _d(absum).reshape(ref.shape)
    err = np.abs(got - ref)
    w = WORST.setdefault(kernel, [0.0, 0.0])
    w[1] = max(w[1], float(np.nanmax(err / (absum + 1e-300) * (absum > 0))) if ref.size else 0.0)
    bad = ~(err <= factor * absum + extra + 1e-30)
    assert not bad.any(), (f"{kernel} {what}: {int(bad.sum())}/{bad.size} outside {factor:g} * sum|terms|; worst "
                           f"{float(np.nanmax(err / (absum + 1e-300))):.3e}")


def _twice(run):
    """Run twice on fresh outputs: bitwise equal (fixed-order reductions)."""
    a, b = run(), run()
    for x, y in zip(a, b):
        assert torch.equal(x, y) or bool((torch.isnan(x) == torch.isnan(y)).all() and
                                         torch.equal(torch.nan_to_num(x), torch.nan_to_num(y))), "not deterministic"
    return a


def _ws(n):
    return torch.empty(max(int(n), 256), dtype=torch.uint8, device="cuda")


# ------------------------------------------------------------------ BN
@pytest.mark.gpu
@pytest.mark.parametrize("D", [1, 37])
@pytest.mark.parametrize("B", [1, 2, 255, 256, 257, 600])
def test_bn_train_fwd_bwd(gpu, B, D):
    """Column 0 has a large mean (1e3 + N(0,1)): a one-pass E[x^2] - E[x]^2 in
    fp32 would lose the variance; column 1 (D > 1) is constant (variance 0).
    mean / var are batch sums (SUM_TOL * sum |terms|).  y is checked twice: as
    the element-wise map of the kernel's own mean / var (1e-5), and against the
    fp64 chain with the mean's bound carried through: y's error from the mean
    is at most SUM_TOL (|x| + mean|x|) |gamma| rsqrt(var + eps)."""
    rng = np.random.default_rng(100 * B + D)
    eps, mom, st = 1e-3, 0.99, _lib.stream()
    x = _nrm(rng, B, D)
    x[:, 0] += 1e3
    if D > 1:
        x[:, 1] = 1.5
    gamma, beta, dy = _nrm(rng, D), _nrm(rng, D), _nrm(rng, B, D)
    mm0, mv0 = _nrm(rng, D), rng.random(D).astype(F32)
    mean64, var64 = ref_bn_stats(x)
    for pad in (0, 3):
        for mov_mean, mov_var in ((True, True), (True, False), (False, True), (False, False)):
            xd, gd, bd = _rows(x, pad), _dev(gamma), _dev(beta)

            def run():
                mm, mv = _dev(mm0), _dev(mv0)
                mean, var, y = _out(1, D), _out(1, D), _out(B, D, pad)
                _lib.call("rs_bn_train_fwd", xd.data_ptr(), D + pad, B, D, gd.data_ptr(), bd.data_ptr(), eps, mom,
                          mm.data_ptr() if mov_mean else None, mv.data_ptr() if mov_var else None, mean.data_ptr(),
                          var.data_ptr(), y.data_ptr(), D + pad, st)
                return mean, var, y, mm, mv

            mean, var, y, mm, mv = _twice(run)
            ax = np.abs(_d(x))
            _sum_close("rs_bn_train_fwd", mean, mean64[None], ax.mean(0)[None], "mean")
            _sum_close("rs_bn_train_fwd", var, var64[None], var64[None], "var")
            km, kv = _get(mean)[0], _get(var)[0]
            yk = _get(y, D)
            _close("rs_bn_train_fwd", yk, ref_bn_apply(x, km, kv, gamma, beta, eps), "y from the kernel's statistics")
            y64 = ref_bn_apply(x, mean64, var64, gamma, beta, eps)
            carried = (ax + ax.mean(0)) * np.abs(_d(gamma)) / np.sqrt(var64 + eps)
            rms = float(np.sqrt(np.mean(y64 ** 2)))
            _sum_close("rs_bn_train_fwd (y, fp64 chain)", yk, y64, carried, "y",
                       extra=RTOL * np.maximum(np.abs(y64), rms))
            if mov_mean:
                _close("rs_bn_train_fwd", mm, mom * _d(mm0) + (1 - mom) * _d(km), "moving mean")
            else:
                assert np.array_equal(_get(mm), mm0)
            if mov_var:
                _close("rs_bn_train_fwd", mv, mom * _d(mv0) + (1 - mom) * _d(kv), "moving var")
            else:
                assert np.array_equal(_get(mv), mv0)

        # backward from the fp32 statistics the forward would hand over
        m32, v32 = mean64.astype(F32), var64.astype(F32)
        md, vd, dyd = _dev(m32), _dev(v32), _rows(dy, pad)

        def run_b():
            dx, dg, db = _out(B, D, pad), _out(1, D), _out(1, D)
            _lib.call("rs_bn_train_bwd", xd.data_ptr(), D + pad, B, D, md.data_ptr(), vd.data_ptr(), gd.data_ptr(),
                      eps, dyd.data_ptr(), D + pad, dx.data_ptr(), D + pad, dg.data_ptr(), db.data_ptr(), st)
            return dx, dg, db

        dx, dg, db = _twice(run_b)
        r, a = ref_bn_bwd(x, m32, v32, gamma, eps, dy), ref_bn_bwd(x, m32, v32, gamma, eps, dy, ab=True)
        _sum_close("rs_bn_train_bwd", _get(dx, D), r[0], a[0], "dx")
        _sum_close("rs_bn_train_bwd", dg, r[1][None], a[1][None], "dgamma")
        _sum_close("rs_bn_train_bwd", db, r[2][None], a[2][None], "dbeta")


# ------------------------------------------------- masked softmax + pool
def _pool_case(rng, B, T, K, variant):
    score = (3 * rng.standard_normal((B, T))).astype(F32)
    seq, datt = _nrm(rng, B, T, K), _nrm(rng, B, K)
    live = rng.random((B, T)) < 0.6
    special = [0, 1, 2] if B >= 3 else [variant % 3]
    for b, kind in enumerate(special):
        live[b] = kind == 2                 # 0: fully padded, 2: fully live
        if kind == 1:
            live[b, T // 2] = True          # a single live position
    ids = np.where(live, rng.integers(1, 1000, (B, T)), 0)
    return score, seq, datt, live, ids, special


@pytest.mark.gpu
@pytest.mark.parametrize("hist_dtype", [np.int32, np.int64, np.float32])
@pytest.mark.parametrize("K", [1, 8, 32, 3, 24, 64, 100])
def test_masked_softmax_pool_fwd_bwd(gpu, K, hist_dtype):
    """K = 1, 8, 32: the lane-group branch (K < 64 dividing 64); K = 3, 24, 64,
    100: a lane per column (100: two rounds of 64 columns).  T = 63 / 64 / 65 /
    130 / 512: a partial, a full, 1 + 1/64, 2 + 2/64 and all 8 chunks of 64
    positions.  B = 1, 5, 9: the last block of 4 waves has idle waves."""
    st, kind = _lib.stream(), {np.int32: 0, np.int64: 1, np.float32: 2}[hist_dtype]
    rng = np.random.default_rng(1000 * K + kind)
    for ti, T in enumerate([1, 63, 64, 65, 130, 512]):
        for B in (1, 5, 9):
            score, seq, datt, live, ids, special = _pool_case(rng, B, T, K, ti + K)
            a64, out64 = ref_pool(score, live, seq)
            sd, qd = _dev(score), _dev(seq)
            for pad in (0, 3):
                fill = np.nan if hist_dtype is np.float32 else 7  # padding read as a mask would be "live"
                hd = _rows(ids, pad, fill, hist_dtype)

                def run():
                    a, out = _out(B, T), _out(B, K, pad)
                    _lib.call("rs_masked_softmax_pool", sd.data_ptr(), hd.data_ptr(), kind, T + pad, qd.data_ptr(),
                              B, T, K, a.data_ptr(), out.data_ptr(), K + pad, st)
                    return a, out

                a, out = _twice(run)
                what = f"T={T} B={B} pad={pad}"
                _close("rs_masked_softmax_pool", a, a64, "a " + what)
                _close("rs_masked_softmax_pool", _get(out, K), out64, "out " + what)
                ak = _get(a)
                for b in range(B):
                    if live[b].any():
                        assert np.all(ak[b][~live[b]] == 0.0), f"masked weight not exactly 0 ({what}, row {b})"
                    else:
                        np.testing.assert_allclose(ak[b], 1.0 / T, rtol=RTOL, err_msg=what)

                # backward from the reference's weights rounded to fp32
                a32 = a64.astype(F32)
                ad, dd = _dev(a32), _rows(datt, pad)

                def run_b():
                    ds, dseq = _out(B, T), _out(B * T, K)
                    _lib.call("rs_masked_softmax_pool_bwd", ad.data_ptr(), hd.data_ptr(), kind, T + pad,
                              qd.data_ptr(), dd.data_ptr(), K + pad, B, T, K, ds.data_ptr(), dseq.data_ptr(), st)
                    return ds, dseq

                ds, dseq = _twice(run_b)
                ds64, dseq64 = ref_pool_bwd(a32, live, seq, datt)
                _close("rs_masked_softmax_pool_bwd", ds, ds64, "ds " + what)
                _close("rs_masked_softmax_pool_bwd", dseq, dseq64.reshape(B * T, K), "dseq (stored) " + what)
                assert np.all(_get(ds)[~live] == 0.0)


# ------------------------------------------------------ attention concat
@pytest.mark.gpu
@pytest.mark.parametrize("K", [4, 16, 256, 3, 24, 300])
def test_din_att_concat_fwd_bwd(gpu, K):
    """K = 4, 16, 256 divide 256: one block per sample (256: a lane per
    column); K = 3, 24, 300: the generic kernel.  dq is a column range of a
    wider matrix (the model's dx + 4K) and is added to, as is dseq."""
    st = _lib.stream()
    rng = np.random.default_rng(K)
    for T in (1, 7, 100):
        for B in (1, 5):
            q, s, d = _nrm(rng, B, K), _nrm(rng, B, T, K), _nrm(rng, B * T, 4 * K)
            what = f"T={T} B={B}"
            qd, sd, dd = _dev(q), _dev(s), _dev(d)

            def run_f():
                out = _out(B * T, 4 * K)
                _lib.call("rs_din_att_concat", qd.data_ptr(), sd.data_ptr(), B, T, K, out.data_ptr(), st)
                return (out,)

            _close("rs_din_att_concat", _twice(run_f)[0], ref_concat(q, s).reshape(B * T, 4 * K), what)
            dq64, dseq64 = ref_concat_bwd(d.reshape(B, T, 4 * K), q, s)
            for off, wide in ((0, K), (5, K + 5 + 3)):  # dense rows; columns [5, 5 + K) of a wider matrix
                dq0, dseq0 = _nrm(rng, B, K), _nrm(rng, B * T, K)
                buf0 = np.full((B, wide), SENT, F32)
                buf0[:, off:off + K] = dq0

                def run():
                    buf, dseq = _dev(buf0), _dev(dseq0)
                    _lib.call("rs_din_att_concat_bwd", dd.data_ptr(), qd.data_ptr(), sd.data_ptr(), B, T, K,
                              buf.data_ptr() + 4 * off, wide, dseq.data_ptr(), st)
                    return buf, dseq

                buf, dseq = _twice(run)
                got = _get(buf)
                assert np.all(got[:, :off] == SENT) and np.all(got[:, off + K:] == SENT), "dq left its columns"
                _close("rs_din_att_concat_bwd", got[:, off:off + K], _d(dq0) + dq64, "dq += " + what)
                _close("rs_din_att_concat_bwd", dseq, _d(dseq0) + dseq64.reshape(B * T, K), "dseq += " + what)


# ------------------------------------------------------------ PReLU rows
@pytest.mark.gpu
@pytest.mark.parametrize("M,N,period", [(5, 3, 1), (300, 65, 1), (6 * 7, 20, 7), (3 * 128, 128, 128)])
def test_prelu_rows_fwd_bwd(gpu, M, N, period):
    """alpha[(r mod period), c]; z exactly 0 takes the alpha branch of dz and
    contributes 0 to dalpha, as the reference's z > 0 and min(z, 0).  The last
    case sums 16384 columns of the [M / period, period * N] view."""
    st = _lib.stream()
    rng = np.random.default_rng(M + N)
    z, dy, alpha = _nrm(rng, M, N), _nrm(rng, M, N), _nrm(rng, period, N)
    z[rng.random((M, N)) < 0.05] = 0.0
    z[0, 0] = 0.0
    zd, dyd, ad = _dev(z), _dev(dy), _dev(alpha)

    def run_f():
        y = _out(M, N)
        _lib.call("rs_prelu_rows_fwd", zd.data_ptr(), M, N, ad.data_ptr(), period, y.data_ptr(), st)
        return (y,)

    _close("rs_prelu_rows_fwd", _twice(run_f)[0], ref_prelu_rows(z, alpha, period), "y")
    ws = _ws(_lib.lib().rs_prelu_rows_bwd_workspace_size(M, N, period))

    def run():
        dz, dal = _out(M, N), _out(period, N)
        _lib.call("rs_prelu_rows_bwd", zd.data_ptr(), dyd.data_ptr(), M, N, ad.data_ptr(), period, dz.data_ptr(),
                  dal.data_ptr(), ws.data_ptr(), ws.numel(), st)
        return dz, dal

    dz, dal = _twice(run)
    r, a = ref_prelu_rows_bwd(z, dy, alpha, period), ref_prelu_rows_bwd(z, np.abs(dy), alpha, period, ab=True)
    _close("rs_prelu_rows_bwd", dz, r[0], "dz")
    assert np.array_equal(_get(dz)[z == 0], (dy * _alpha_rows(alpha, M, N, period).astype(F32))[z == 0])
    _sum_close("rs_prelu_rows_bwd", dal, r[1], a[1], "dalpha")


# ------------------------------------- the one-launch PReLU attention unit
def _gemm(ta, tb, M, N, K, A, B_, Cout, ws, st):
    _lib.call("rs_gemm", ta, tb, M, N, K, 1.0, A.data_ptr(), A.stride(0), B_.data_ptr(), B_.stride(0), 0.0,
              Cout.data_ptr(), N, None, 0, ws.data_ptr(), ws.numel(), st)


def _att_layered(h0, z1, z2, ds, W1, W2, al1, al2, wo, T, st):
    """The unit's backward layer by layer on the device (DIN.train_step's path
    for shapes the one-launch kernel refuses)."""
    M, K0 = h0.shape
    h1, h2 = W2.shape
    lb = _lib.lib()
    ws = _ws(max(lb.rs_gemm_workspace_size(K0, h1, M), lb.rs_gemm_workspace_size(h1, h2, M),
                 lb.rs_gemm_workspace_size(h2, 1, M), lb.rs_col_sum_workspace_size(M, max(h1, h2)),
                 lb.rs_prelu_rows_bwd_workspace_size(M, max(h1, h2), T)))
    emp = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device="cuda")
    y1, y2 = emp(M, h1), emp(M, h2)
    _lib.call("rs_prelu_rows_fwd", z1.data_ptr(), M, h1, al1.data_ptr(), T, y1.data_ptr(), st)
    _lib.call("rs_prelu_rows_fwd", z2.data_ptr(), M, h2, al2.data_ptr(), T, y2.data_ptr(), st)
    colsum = lambda A, n, out: _lib.call("rs_col_sum_split", A.data_ptr(), n, M, n, out.data_ptr(), ws.data_ptr(),
                                         ws.numel(), st)
    dwo, dbo, dy2 = emp(h2), emp(1), emp(M, h2)
    _gemm(1, 0, h2, 1, M, y2, ds.view(M, 1), dwo, ws, st)
    colsum(ds, 1, dbo)
    _gemm(0, 1, M, h2, 1, ds.view(M, 1), wo.view(h2, 1), dy2, ws, st)
    dz2, dal2, dW2, db2, dy1 = emp(M, h2), emp(T, h2), emp(h1, h2), emp(h2), emp(M, h1)
    _lib.call("rs_prelu_rows_bwd", z2.data_ptr(), dy2.data_ptr(), M, h2, al2.data_ptr(), T, dz2.data_ptr(),
              dal2.data_ptr(), ws.data_ptr(), ws.numel(), st)
    _gemm(1, 0, h1, h2, M, y1, dz2, dW2, ws, st)
    colsum(dz2, h2, db2)
    _gemm(0, 1, M, h1, h2, dz2, W2, dy1, ws, st)
    dz1, dal1, dW1, db1, dh0 = emp(M, h1), emp(T, h1), emp(K0, h1), emp(h1), emp(M, K0)
    _lib.call("rs_prelu_rows_bwd", z1.data_ptr(), dy1.data_ptr(), M, h1, al1.data_ptr(), T, dz1.data_ptr(),
              dal1.data_ptr(), ws.data_ptr(), ws.numel(), st)
    _gemm(1, 0, K0, h1, M, h0, dz1, dW1, ws, st)
    colsum(dz1, h1, db1)
    _gemm(0, 1, M, K0, h1, dz1, W1, dh0, ws, st)
    return dh0, dW1, db1, dal1, dW2, db2, dal2, dwo, dbo


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 3, 257])
@pytest.mark.parametrize("T,K0,h1,h2", [(1, 4, 4, 4), (17, 12, 20, 12), (20, 16, 80, 40), (100, 32, 80, 40),
                                        (30, 64, 80, 40), (64, 128, 64, 64), (128, 64, 64, 32)])
def test_din_att_prelu_unit_fwd_bwd(gpu, T, K0, h1, h2, B):
    """The one-launch unit against the fp64 unit and against the layer-by-layer
    device path.  Widths 4, 12, 20 are multiples of 4 but not of 16: the MFMA
    tiles' zero pads and row clamps carry them.  B = 257 > the 256 workgroups:
    one of them takes two samples.  The backward gets the reference's z1 / z2
    rounded to fp32, so both sides take the same side of every PReLU kink.
    Two fp32 paths each within a bound of the fp64 value differ by at most
    twice that bound."""
    st, lb = _lib.stream(), _lib.lib()
    rng = np.random.default_rng(T * 1000 + K0 * 10 + B)
    M = B * T
    h0 = _nrm(rng, M, K0)
    W1, b1, al1 = _nrm(rng, K0, h1) / F32(np.sqrt(K0)), 0.1 * _nrm(rng, h1), rng.random((T, h1)).astype(F32)
    W2, b2, al2 = _nrm(rng, h1, h2) / F32(np.sqrt(h1)), 0.1 * _nrm(rng, h2), rng.random((T, h2)).astype(F32)
    wo, bo, ds = _nrm(rng, h2) / F32(np.sqrt(h2)), _nrm(rng, 1), _nrm(rng, M)
    dv = {k: _dev(v) for k, v in dict(h0=h0, W1=W1, b1=b1, al1=al1, W2=W2, b2=b2, al2=al2, wo=wo, bo=bo, ds=ds).items()}
    p = lambda k: dv[k].data_ptr()

    def run_f():
        z1, z2, sc = _out(M, h1), _out(M, h2), _out(1, M)
        _lib.call("rs_din_att_prelu_fwd", p("h0"), p("W1"), p("b1"), p("al1"), p("W2"), p("b2"), p("al2"), p("wo"),
                  p("bo"), B, T, K0, h1, h2, z1.data_ptr(), z2.data_ptr(), sc.data_ptr(), st)
        return z1, z2, sc

    z1, z2, sc = _twice(run_f)
    r1, r2, rs = ref_att_fwd(h0, W1, b1, al1, W2, b2, al2, wo, bo, T)
    _close("rs_din_att_prelu_fwd", z1, r1, "z1")
    _close("rs_din_att_prelu_fwd", z2, r2, "z2")
    _close("rs_din_att_prelu_fwd", sc, rs[None], "score")
    # layer by layer: rs_dense_fwd / rs_prelu_rows_fwd
    emp = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device="cuda")
    lz1, ly1, lz2, ly2, lsc = emp(M, h1), emp(M, h1), emp(M, h2), emp(M, h2), emp(M)
    dense = lambda x, W, b, y, K, N: _lib.call("rs_dense_fwd", x.data_ptr(), K, W.data_ptr(), b.data_ptr(), None,
                                               _lib.ACT[None], y.data_ptr(), N, M, K, N, st)
    dense(dv["h0"], dv["W1"], dv["b1"], lz1, K0, h1)
    _lib.call("rs_prelu_rows_fwd", lz1.data_ptr(), M, h1, p("al1"), T, ly1.data_ptr(), st)
    dense(ly1, dv["W2"], dv["b2"], lz2, h1, h2)
    _lib.call("rs_prelu_rows_fwd", lz2.data_ptr(), M, h2, p("al2"), T, ly2.data_ptr(), st)
    dense(ly2, dv["wo"], dv["bo"], lsc, h2, 1)
    _close("rs_din_att_prelu_fwd", z1, _get(lz1), "z1 against the layered path", rtol=2 * RTOL)
    _close("rs_din_att_prelu_fwd", z2, _get(lz2), "z2 against the layered path", rtol=2 * RTOL)
    _close("rs_din_att_prelu_fwd", sc, _get(lsc)[None], "score against the layered path", rtol=2 * RTOL)

    z1_32, z2_32 = r1.astype(F32), r2.astype(F32)
    z1d, z2d = _dev(z1_32), _dev(z2_32)
    ws = _ws(lb.rs_din_att_prelu_bwd_workspace_size(B, T, K0, h1, h2))
    shapes = [(M, K0), (K0, h1), (1, h1), (T, h1), (h1, h2), (1, h2), (T, h2), (1, h2), (1, 1)]

    def run_b():
        outs = [_out(*s) for s in shapes]
        _lib.call("rs_din_att_prelu_bwd", p("h0"), z1d.data_ptr(), z2d.data_ptr(), p("ds"), p("W1"), p("W2"),
                  p("al1"), p("al2"), p("wo"), B, T, K0, h1, h2, *[o.data_ptr() for o in outs], ws.data_ptr(),
                  ws.numel(), st)
        return outs

    outs = _twice(run_b)
    ref = ref_att_bwd(h0, z1_32, z2_32, ds, W1, W2, al1, al2, wo, T)
    absum = ref_att_bwd(h0, z1_32, z2_32, ds, W1, W2, al1, al2, wo, T, ab=True)
    lay = _att_layered(dv["h0"], z1d, z2d, dv["ds"], dv["W1"], dv["W2"], dv["al1"], dv["al2"], dv["wo"], T, st)
    _close("rs_din_att_prelu_bwd", outs[0], ref[0], "dh0")
    _close("rs_din_att_prelu_bwd", outs[0], _get(lay[0]), "dh0 against the layered path", rtol=2 * RTOL)
    for name, o, r, a, l in list(zip(ATT_NAMES, outs, ref, absum, lay))[1:]:
        _sum_close("rs_din_att_prelu_bwd", o, r, a, name)
        _sum_close("rs_din_att_prelu_bwd", o, _get(l).reshape(np.shape(r)), a, name + " against the layered path",
                   factor=2 * SUM_TOL)


# --------------------------------------------------------------- CrossNet
@pytest.mark.gpu
@pytest.mark.parametrize("d", [1, 63, 64, 65, 429, 2048])
def test_cross_train_fwd_bwd(gpu, d):
    """d = 63 / 64 / 65: a partial wave, a full one, one element into the second
    register; 2048 fills all 32 registers per lane.  Weights scaled by 1/sqrt(d)
    keep x_L O(1).  xl_out is optional; dx is added to; L = 0: dx += dxl."""
    st = _lib.stream()
    rng = np.random.default_rng(d)
    for L in (1, 3):
        for B in (1, 5, 9):
            x0, dxl, dx0 = _nrm(rng, B, d), _nrm(rng, B, d), _nrm(rng, B, d)
            W, b = _nrm(rng, L, d) / F32(np.sqrt(d)), 0.1 * _nrm(rng, L, d)
            Wd, bd = _dev(W), _dev(b)
            xs64, g64, xl64 = ref_cross_fwd(x0, W, b)
            g32 = g64.astype(F32)
            deltas64, s64, add64 = ref_cross_bwd(x0, W, g32, dxl)
            for pad in (0, 3):
                what = f"L={L} B={B} pad={pad}"
                xd = _rows(x0, pad)
                for with_xl in (True, False):
                    def run():
                        xs, g, xl = _out(L * B, d), _out(L, B), _out(B, d, pad)
                        _lib.call("rs_cross_train_fwd", xd.data_ptr(), d + pad, d, L, Wd.data_ptr(), bd.data_ptr(),
                                  B, xs.data_ptr(), g.data_ptr(), xl.data_ptr() if with_xl else None, d + pad, st)
                        return xs, g, xl

                    xs, g, xl = _twice(run)
                    _close("rs_cross_train_fwd", xs, xs64.reshape(L * B, d), "xs " + what)
                    _close("rs_cross_train_fwd", g, g64, "g " + what)
                    if with_xl:
                        _close("rs_cross_train_fwd", _get(xl, d), xl64, "xl_out " + what)
                    else:
                        assert bool(torch.isnan(xl[:, :d]).all())
                gd, dld = _dev(g32), _rows(dxl, pad)

                def run_b():
                    deltas, s, dx = _out(L * B, d), _out(L, B), _out(B, d, pad, dx0)
                    _lib.call("rs_cross_train_bwd", xd.data_ptr(), d + pad, d, L, Wd.data_ptr(), B, gd.data_ptr(),
                              dld.data_ptr(), d + pad, deltas.data_ptr(), s.data_ptr(), dx.data_ptr(), d + pad, st)
                    return deltas, s, dx

                deltas, s, dx = _twice(run_b)
                _close("rs_cross_train_bwd", deltas, deltas64.reshape(L * B, d), "deltas " + what)
                _close("rs_cross_train_bwd", s, s64, "s " + what)
                _close("rs_cross_train_bwd", _get(dx, d), _d(dx0) + add64, "dx += " + what)
    # no cross layer: the output Dense's gradient goes straight to dx
    x0, dxl, dx0 = _nrm(rng, 5, d), _nrm(rng, 5, d), _nrm(rng, 5, d)
    xd, dld, dx = _rows(x0, 3), _rows(dxl, 3), _out(5, d, 3, dx0)
    _lib.call("rs_cross_train_bwd", xd.data_ptr(), d + 3, d, 0, None, 5, None, dld.data_ptr(), d + 3, None, None,
              dx.data_ptr(), d + 3, st)
    _close("rs_cross_train_bwd", _get(dx, d), _d(dx0) + _d(dxl), "L=0 dx += dxl")


# ------------------------------------------- inner product, Bi-Interaction
@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 6])
@pytest.mark.parametrize("F,k", [(2, 1), (3, 5), (26, 16), (64, 64), (64, 3), (5, 64)])
def test_inner_product_bwd(gpu, F, k, B):
    """dflat and dinner are two column ranges of one matrix [flat | inner], as
    PNN.train_step passes the DNN's input gradient; (64, 64) stages the full
    4096 floats and 2016 pair gradients of a sample in LDS."""
    st = _lib.stream()
    rng = np.random.default_rng(F * 100 + k + B)
    P, n = F * (F - 1) // 2, F * k
    e, delta = _nrm(rng, B, n), _nrm(rng, B, n + P)
    for pad in (0, 3):
        ed, dd = _rows(e, pad), _rows(delta, pad)

        def run():
            de = _out(B, n, pad)
            _lib.call("rs_inner_product_bwd", ed.data_ptr(), n + pad, dd.data_ptr() + 4 * n, n + P + pad,
                      dd.data_ptr(), n + P + pad, F, k, B, de.data_ptr(), n + pad, st)
            return (de,)

        de, = _twice(run)
        ref = ref_inner_bwd(e.reshape(B, F, k), delta[:, n:], delta[:, :n].reshape(B, F, k))
        _close("rs_inner_product_bwd", _get(de, n), ref.reshape(B, n), f"demb pad={pad}")


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 300])
@pytest.mark.parametrize("F,k", [(1, 1), (26, 8), (39, 5)])
def test_bi_interaction_bwd(gpu, F, k, B):
    st = _lib.stream()
    rng = np.random.default_rng(F + k + B)
    e, dbi = _nrm(rng, B, F * k), _nrm(rng, B, k)
    for pad in (0, 3):
        ed, dd = _rows(e, pad), _rows(dbi, pad)

        def run():
            de = _out(B, F * k, pad)
            _lib.call("rs_bi_interaction_bwd", ed.data_ptr(), F * k + pad, dd.data_ptr(), k + pad, F, k, B,
                      de.data_ptr(), F * k + pad, st)
            return (de,)

        de, = _twice(run)
        _close("rs_bi_interaction_bwd", _get(de, F * k), ref_bi_bwd(e.reshape(B, F, k), dbi).reshape(B, F * k),
               f"demb pad={pad}")


# ---------------------------------------------------------------- losses
@pytest.mark.gpu
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("B", [1, 1023, 1024, 1025, 3000])
def test_bce_prob_grad(gpu, B, stride):
    """One workgroup of 1024: B = 1023 / 1024 / 1025 / 3000 are under, at, over
    and three rounds.  Outside the clip range g is exactly 0; for p >= 1 the
    term 1 - q + eps is below fp32 resolution, so only g == 0 and a finite loss
    are required there."""
    st = _lib.stream()
    rng = np.random.default_rng(B)
    pre = rng.uniform(0.01, 0.99, B).astype(F32)
    if B > 4:
        pre[:4] = [-0.3, 0.0, 1.0, 1.7]
    elif stride == 1:
        pre[:] = 0.0  # B = 1: the lower clip edge alone; stride 2 keeps the interior draw
    t = rng.integers(0, 2, B).astype(F32)
    pd, td = _rows(pre[:, None], stride - 1), _dev(t)
    g64, loss64 = ref_bce_prob(pre, t)
    for with_loss in (True, False):
        def run():
            g, loss = _out(1, B), _out(1, B)
            _lib.call("rs_bce_prob_grad", pd.data_ptr(), stride, td.data_ptr(), B, g.data_ptr(),
                      loss.data_ptr() if with_loss else None, st)
            return g, loss

        g, loss = _twice(run)
        _close("rs_bce_prob_grad", g, g64[None], "g")
        outside = (pre <= 0) | (pre >= 1)
        assert np.all(_get(g)[0][outside] == 0.0)
        if with_loss:
            lk = _get(loss)[0]
            assert np.all(np.isfinite(lk))
            keep = pre < 1
            if keep.any():
                _close("rs_bce_prob_grad", lk[keep], loss64[keep], "loss")
        else:
            assert bool(torch.isnan(loss).all())


@pytest.mark.gpu
@pytest.mark.parametrize("c_fm,c_dnn", [(0.5, 0.5), (1.0, 0.0)])
@pytest.mark.parametrize("B", [1, 256, 257])
def test_head_grad(gpu, B, c_fm, c_dnn):
    st = _lib.stream()
    rng = np.random.default_rng(B)
    fm, dnn = (20 * rng.standard_normal(B)).astype(F32), (20 * rng.standard_normal(B)).astype(F32)
    if B > 4:
        fm[:4], dnn[:4] = [40, -40, 40, -40], [40, -40, 40, -40]
    t = rng.integers(0, 2, B).astype(F32)
    if B > 4:
        t[:4] = [1, 1, 0, 0]
    fd, dd, td = _dev(fm), _dev(dnn), _dev(t)
    r = ref_head(fm, dnn, t, c_fm, c_dnn)
    for with_loss in (True, False):
        def run(scaled=False):
            gf, gd, loss = _out(1, B), _out(1, B), _out(1, B)
            lp = loss.data_ptr() if with_loss else None
            if scaled:
                _lib.call("rs_head_grad_scaled", fd.data_ptr(), dd.data_ptr(), td.data_ptr(), B, c_fm, c_dnn,
                          1.0 / B, gf.data_ptr(), gd.data_ptr(), lp, st)
            else:
                _lib.call("rs_head_grad", fd.data_ptr(), dd.data_ptr(), td.data_ptr(), B, c_fm, c_dnn,
                          gf.data_ptr(), gd.data_ptr(), lp, st)
            return gf, gd, loss

        outs, outs_s = _twice(run), run(True)
        for o, os_, ref, name in zip(outs, outs_s, r, ("g_fm", "g_dnn", "loss")):
            if name == "loss" and not with_loss:
                assert bool(torch.isnan(o).all())
                continue
            _close("rs_head_grad", o, ref[None], name)
            _close("rs_head_grad_scaled", os_, ref[None], name + " (scale = 1/B)")
            _close("rs_head_grad_scaled", os_, _get(o), name + " against rs_head_grad")


# ------------------------------------------------------------------- FFM
@pytest.mark.gpu
@pytest.mark.parametrize("id_dtype", [np.int32, np.int64, np.float32])
@pytest.mark.parametrize("B", [1, 6])
@pytest.mark.parametrize("nd,F,k", [(0, 1, 1), (13, 26, 8), (3, 70, 4), (0, 64, 64)])
def test_ffm_train_fwd(gpu, nd, F, k, B, id_dtype):
    """(3, 70, 4): more than 64 fields + dense features (two rounds of the
    linear part); (0, 64, 64): E = 4096, the whole LDS slot of a wave.  One
    id per batch is out of range: tf.one_hot's zero row, no failure."""
    st = _lib.stream()
    rng = np.random.default_rng(nd + 10 * F + k + B)
    vocab = rng.integers(2, 6, F)
    offs = np.concatenate([[0], np.cumsum(vocab)[:-1]]).astype(np.int64)
    n_feat, NF = nd + int(vocab.sum()), nd + F
    E = NF * k
    v = _nrm(rng, n_feat, NF, k)
    w, w0 = 0.1 * _nrm(rng, n_feat, 1), 0.1 * _nrm(rng, 1)
    dense = rng.random((B, nd)).astype(F32)
    ids = np.stack([rng.integers(0, n, B) for n in vocab], 1)
    ids[0, F // 2] = vocab[F // 2]  # one past the field's last id
    t = rng.integers(0, 2, B).astype(F32)
    # z is quadratic in v: scale v so that the logits are O(1)
    with np.errstate(over="ignore"):  # the unscaled logits overflow the reference's exp; only z is used
        zmax = np.abs(ref_ffm_train(dense, ids, vocab, 0 * w0, 0 * w, v, t)[3]).max()
    v = (v / F32(np.sqrt(max(zmax, 1e-3)))).astype(F32)
    G64, g64, loss64, _ = ref_ffm_train(dense, ids, vocab, w0, w, v, t)
    kind = {np.int32: 0, np.int64: 1, np.float32: 2}[id_dtype]
    for pad in (0, 3):
        idd = _rows(ids, pad, np.nan if id_dtype is np.float32 else -5, id_dtype)
        dd = _rows(dense, pad) if nd else None
        vd, wd, w0d, od, vod, td = _dev(v), _dev(w), _dev(w0), _dev(offs, np.int64), _dev(vocab, np.int64), _dev(t)
        for with_loss in (True, False):
            def run():
                G, g, loss = _out(B, E), _out(1, B), _out(1, B)
                _lib.call("rs_ffm_train_fwd", idd.data_ptr(), kind, F + pad, dd.data_ptr() if nd else None, nd + pad,
                          nd, vd.data_ptr(), wd.data_ptr(), w0d.data_ptr(), od.data_ptr(), vod.data_ptr(), F, k,
                          td.data_ptr(), B, G.data_ptr(), g.data_ptr(), loss.data_ptr() if with_loss else None, st)
                return G, g, loss

            G, g, loss = _twice(run)
            _close("rs_ffm_train_fwd", G, G64, "G")
            _close("rs_ffm_train_fwd", g, g64[None], "g")
            if with_loss:
                _close("rs_ffm_train_fwd", loss, loss64[None], "loss")
            else:
                assert bool(torch.isnan(loss).all())


# ------------------------------------------------------------- l2 decay
@pytest.mark.gpu
@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("n", [1, 3, 4, 1023, 1024, 4100])
def test_l2_decay(gpu, n, offset):
    """w -= lr 2 l2 w.  n % 4 != 0, or a pointer one float into an aligned
    tensor, takes the scalar path for every element; the floats around the
    range stay untouched."""
    st = _lib.stream()
    rng = np.random.default_rng(n)
    lr, l2 = 0.05, 0.3
    w0 = _nrm(rng, n)
    buf0 = np.full(offset + n + 5, SENT, F32)
    buf0[offset:offset + n] = w0

    def run():
        buf = _dev(buf0)
        _lib.call("rs_l2_decay", buf.data_ptr() + 4 * offset, n, lr, l2, st)
        return (buf,)

    buf, = _twice(run)
    got = buf.cpu().numpy()
    assert np.all(got[:offset] == SENT) and np.all(got[offset + n:] == SENT)
    f = float(F32(lr) * F32(2.0) * F32(l2))
    _close("rs_l2_decay", got[offset:offset + n], _d(w0) * (1.0 - f), "w")


# ----------------------------------------------------- row-sparse SGD
@pytest.mark.gpu
@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("k", [1, 5])
def test_embedding_sgd_strided(gpu, k, shared):
    """grad_field_stride = k (a gradient row per lookup) and 0 (a row per
    sample shared by its fields, the FFM step).  Row 2 takes more than half
    of the 900 lookups, so its sum crosses the 256-lookup chunks; one id is
    out of range: skipped, and the error flag is raised."""
    st, lb = _lib.stream(), _lib.lib()
    rng = np.random.default_rng(k + 7 * shared)
    B, vocab, lr = 300, np.array([5, 5, 4]), 0.5
    F, n_rows = len(vocab), 9
    offs = np.array([0, 0, 5], np.int64)  # fields 0 and 1 share their rows (as DIN's candidate and history)
    ids = np.stack([rng.integers(0, n, B) for n in vocab], 1).astype(np.int32)
    ids[:, 0] = 2  # the hot row: every lookup of field 0 and most of field 1
    ids[rng.random(B) < 0.8, 1] = 2
    ids[7, 1] = vocab[1] + 3  # bad id
    assert ((ids + offs[None, :])[:, :2] == 2).sum() > B * F // 2
    gfs = 0 if shared else k
    gw = k if shared else F * k
    grad, table0 = _nrm(rng, B, gw), _nrm(rng, n_rows, k)
    ref, absum = _d(table0).copy(), np.abs(_d(table0))
    for b in range(B):
        for c in range(F):
            if 0 <= ids[b, c] < vocab[c]:
                gr = _d(grad[b, c * gfs:c * gfs + k])
                ref[offs[c] + ids[b, c]] -= lr * gr
                absum[offs[c] + ids[b, c]] += lr * np.abs(gr)
    od, vod = _dev(offs, np.int64), _dev(vocab, np.int64)
    ws = _ws(lb.rs_embedding_sgd_workspace_size(B * F))
    for pad in (0, 3):
        idd, gd = _rows(ids, pad, -9, np.int32), _rows(grad, pad)

        def run(plain=False, flag=True):
            table, err = _dev(table0), torch.zeros(1, dtype=torch.int32, device="cuda")
            ep = err.data_ptr() if flag else None
            if plain:
                _lib.call("rs_embedding_sgd", table.data_ptr(), n_rows, k, idd.data_ptr(), 0, F + pad, od.data_ptr(),
                          vod.data_ptr(), F, B, gd.data_ptr(), gw + pad, lr, ws.data_ptr(), ep, st)
            else:
                _lib.call("rs_embedding_sgd_strided", table.data_ptr(), n_rows, k, idd.data_ptr(), 0, F + pad,
                          od.data_ptr(), vod.data_ptr(), F, B, gd.data_ptr(), gw + pad, gfs, lr, ws.data_ptr(), ep, st)
            return table, err

        table, err = _twice(run)
        assert int(err.item()) & _lib.FLAG_BAD_ID
        _sum_close("rs_embedding_sgd_strided", table, ref, absum, f"table pad={pad}")
        assert torch.equal(table, run(flag=False)[0]), "err_flag = NULL changes nothing else"
        if not shared:
            assert torch.equal(table, run(True)[0]), "stride k must be rs_embedding_sgd bit for bit"


# ------------------------------------------------------------ FM gradients
@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 257])
@pytest.mark.parametrize("d", [1, 70])
@pytest.mark.parametrize("kfm", [1, 16, 17, 32])
def test_fm_grads(gpu, kfm, d, B):
    """kfm = 1, 16: the KF = 16 instance; 17, 32: KF = 32.  dx is added to; the
    strided form reads s and g out of interleaved [s | g] records and skips
    dw0 when it is NULL."""
    st = _lib.stream()
    rng = np.random.default_rng(kfm * 1000 + d * 3 + B)
    x, w1, v, g = _nrm(rng, B, d), _nrm(rng, d), _nrm(rng, d, kfm) / F32(np.sqrt(kfm)), _nrm(rng, B)
    s = (_d(x) @ _d(v)).astype(F32)
    dx0 = _nrm(rng, B, d)
    r, a = ref_fm_grads(x, s, w1, v, g), ref_fm_grads(x, s, w1, v, g, ab=True)
    sd, w1d, vd, gd = _dev(s), _dev(w1), _dev(v), _dev(g)
    rec = _rows(np.concatenate([s, g[:, None]], 1), 2)  # [s | g | padding]
    for pad in (0, 3):
        xd = _rows(x, pad)

        def run():
            dx, dw1, dv, dw0 = _out(B, d, pad, dx0), _out(1, d), _out(d, kfm), _out(1, 1)
            _lib.call("rs_fm_x_grad", xd.data_ptr(), d + pad, sd.data_ptr(), w1d.data_ptr(), vd.data_ptr(), B, d,
                      kfm, gd.data_ptr(), dx.data_ptr(), d + pad, st)
            _lib.call("rs_fm_param_grads", xd.data_ptr(), d + pad, sd.data_ptr(), vd.data_ptr(), B, d, kfm,
                      gd.data_ptr(), dw1.data_ptr(), dv.data_ptr(), dw0.data_ptr(), st)
            return dx, dw1, dv, dw0

        def run_s(with_dw0):
            dw1, dv, dw0 = _out(1, d), _out(d, kfm), _out(1, 1)
            _lib.call("rs_fm_param_grads_strided", xd.data_ptr(), d + pad, rec.data_ptr(), kfm + 3,
                      rec.data_ptr() + 4 * kfm, kfm + 3, vd.data_ptr(), B, d, kfm, dw1.data_ptr(), dv.data_ptr(),
                      dw0.data_ptr() if with_dw0 else None, st)
            return dw1, dv, dw0

        dx, dw1, dv, dw0 = _twice(run)
        _close("rs_fm_x_grad", _get(dx, d), _d(dx0) + r[0], f"dx += pad={pad}")
        _sum_close("rs_fm_param_grads", dw1, r[1][None], a[1][None], "dw1")
        _sum_close("rs_fm_param_grads", dv, r[2], a[2], "dv")
        _sum_close("rs_fm_param_grads", dw0, r[3][None], a[3][None], "dw0")
        for with_dw0 in (True, False):
            s1, sv, s0 = run_s(with_dw0)
            assert torch.equal(s1, dw1) and torch.equal(sv, dv), "the strided form reads the same values"
            assert torch.equal(s0, dw0) if with_dw0 else bool(torch.isnan(s0).all())
