"""Training of DIEN: the recurrences (dien_train.hip: rs_gru_train_fwd /
rs_augru_train_fwd, rs_gru_bwd / rs_augru_bwd, the host layers'
``train_forward`` / ``backward``) and, in the second half of the file,
``DIEN.train_step`` with the auxiliary loss and ``compile_fit``.

The reference is the training forward restated in torch on the CPU (float64)
with gradients from torch.autograd; it is pinned here against central finite
differences (step 1e-6, agreement 1e-6) and by one GRU and one AUGRU backward
step worked by hand.  For every case a GPU test runs, a CPU test requires the
same restatement in float32 to sit within RTOL / 4 of the float64 one, and the
kink preconditions (no AUGRU gate pre-activation within 1e-3 of +-2.5) are
checked on the reference alone.  GPU tests compare at tests.helpers.RTOL.

The finite-difference, by-hand, conditioning and kink tests exercise only the
restatement in this file: they pin the reference and pass without the feature.
Every other test here (the size queries, the argument refusals, the limits,
auxiliary_nn, and all GPU tests) needs the new entries, layers' methods or
``train_step`` and fails without them."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import recommender_system_amd as rs
from recommender_system_amd import _lib
from tests.helpers import RTOL, assert_scaled_close
from tests.test_dien import augru_ref, dien_ref, gru_ref, rand_evolution_weights, toy_columns

gpu_test = pytest.mark.gpu
LR, STEPS = 0.2, 3  # the model tests' learning rate and number of steps
MASKED = float(-2 ** 32 + 1)
F64 = torch.float64


# ------------------------------------------------------- the restatement
def hsig_t(x):
    return torch.clamp(0.2 * x + 0.5, 0, 1)


def gru_t(x, W, U, b):
    """Keras GRU(reset_after=True), gate order z r h: the sequence [B, T, U]."""
    B, T, _ = x.shape
    u = U.shape[0]
    h = torch.zeros(B, u, dtype=x.dtype)
    out = []
    for t in range(T):
        xi = x[:, t] @ W + b[0]
        hr = h @ U + b[1]
        z = torch.sigmoid(xi[:, :u] + hr[:, :u])
        r = torch.sigmoid(xi[:, u:2 * u] + hr[:, u:2 * u])
        hh = torch.tanh(xi[:, 2 * u:] + r * hr[:, 2 * u:])
        h = z * h + (1 - z) * hh
        out.append(h)
    return torch.stack(out, 1)


def augru_t(x, s, W, U, update="reference", pre=None):
    """AUGRU over AUGRUCell: the last state [B, U]; ``pre`` collects the gate
    pre-activations (a_z, a_r) of every step."""
    B, T, _ = x.shape
    u = U.shape[0]
    h = torch.zeros(B, u, dtype=x.dtype)
    for t in range(T):
        xi = x[:, t] @ W
        az, ar = xi[:, :u] + h @ U[:, :u], xi[:, u:2 * u] + h @ U[:, u:2 * u]
        if pre is not None:
            pre.append((az.detach().numpy().copy(), ar.detach().numpy().copy()))
        z = hsig_t(az) * s[:, t:t + 1]
        r = hsig_t(ar)
        hh = torch.tanh(xi[:, 2 * u:] + (r * h) @ U[:, 2 * u:])
        h = z * h + (1 - z) * hh if update == "reference" else (1 - z) * h + z * hh
    return h


def mask_scores_t(s, lengths, norm):
    """AttentionSequencePoolingLayer's mask: positions t >= len at -2^32 + 1 and
    a softmax over T, or set to 0."""
    T = s.shape[1]
    valid = torch.arange(T)[None] < torch.as_tensor(np.asarray(lengths)).reshape(-1, 1)
    if not norm:
        return torch.where(valid, s, torch.zeros_like(s))
    return torch.softmax(torch.where(valid, s, torch.full_like(s, MASKED)), dim=1)


def scaled_err(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    rms = float(np.sqrt(np.mean(ref ** 2)))
    if rms == 0:  # an all-zero reference (dU at T = 1): only zeros match it
        return 0.0 if not np.any(got) else float("inf")
    return float(np.max(np.abs(got - ref) / np.maximum(np.abs(ref), rms)))


class Case:
    pass


def _t(a, dt):
    return torch.tensor(np.asarray(a), dtype=dt)


GRU_SHAPES = [(1, 1, 16, 16), (17, 2, 12, 12), (33, 7, 12, 12), (17, 20, 36, 36), (5, 7, 8, 12), (5, 7, 20, 12),
              (16, 5, 64, 64), (17, 50, 36, 36)]
GRU_MODES = ("last", "seq", "both")


def _gru_inputs(B, T, din, U):
    rng = np.random.default_rng([1, B, T, din, U])
    c = Case()
    c.B, c.T, c.din, c.U = B, T, din, U
    w = rand_evolution_weights(rng, U, (), "relu", din=din)
    c.W, c.Ur, c.b = w["gru1/kernel"], w["gru1/recurrent_kernel"], w["gru1/bias"]
    c.x = rng.normal(0, 0.5, (B, T, din)).astype(np.float32)
    c.gseq = rng.normal(0, 1, (B, T, U)).astype(np.float32)
    c.glast = rng.normal(0, 1, (B, U)).astype(np.float32)
    return c


def gru_grads(c, mode, dt=F64):
    """(seq, dx, dW, dU, db) of sum(seq * gseq) + sum(seq[:, -1] * glast)."""
    x, W, U, b = (_t(v, dt).requires_grad_() for v in (c.x, c.W, c.Ur, c.b))
    seq = gru_t(x, W, U, b)
    loss = 0
    if mode in ("seq", "both"):
        loss = loss + (seq * _t(c.gseq, dt)).sum()
    if mode in ("last", "both"):
        loss = loss + (seq[:, -1] * _t(c.glast, dt)).sum()
    g = torch.autograd.grad(loss, (x, W, U, b))
    return [seq.detach().numpy()] + [v.numpy() for v in g]


@functools.lru_cache(maxsize=None)
def gru_case(B, T, din, U):
    c = _gru_inputs(B, T, din, U)
    c.ref = {m: gru_grads(c, m) for m in GRU_MODES}
    return c


# (B, T, din, U, norm, update, scale, seed): scale multiplies the AUGRU kernels; the seed is one at which the
# reference meets the preconditions below
SAT_SEED = 4
AUGRU_CASES = [(B, T, din, U, norm, "reference", 1.0, 0) for (B, T, din, U) in GRU_SHAPES for norm in (True, False)] + \
    [(33, 7, 12, 12, True, "paper", 1.0, 0), (33, 7, 12, 12, False, "paper", 1.0, 0),
     (17, 20, 36, 36, True, "paper", 1.0, 0),
     (5, 7, 8, 12, False, "reference", 12.0, SAT_SEED), (5, 7, 8, 12, True, "paper", 12.0, SAT_SEED),
     (5, 7, 8, 12, True, "reference", 12.0, SAT_SEED), (5, 7, 8, 12, False, "paper", 12.0, SAT_SEED)]
SATURATING = [k for k in AUGRU_CASES if k[6] != 1.0]
_aid = lambda k: "-".join(str(v) for v in k)


def _augru_inputs(B, T, din, U, norm, update, scale=1.0, seed=0):
    rng = np.random.default_rng([2, B, T, din, U, int(norm), int(scale), seed])
    c = Case()
    c.B, c.T, c.din, c.U, c.norm, c.update = B, T, din, U, norm, update
    w = rand_evolution_weights(rng, U, (), "relu", din=din)
    # the z and r gates' columns scaled (saturating hsig); the candidate's are not: tanh' = 1 - hh^2 next to
    # hh = +-1 cancels in float32, which would make the case ill-conditioned and say nothing about hsig
    gates = np.concatenate([np.full(2 * U, scale), np.ones(U)]).astype(np.float32)
    c.W, c.Ur = w["gru1/kernel"] * gates, w["gru1/recurrent_kernel"] * gates
    c.x = rng.normal(0, 0.5, (B, T, din)).astype(np.float32)
    # raw scores: negative and above 1 (they reach the AUGRU as they are without normalisation)
    c.raw = rng.normal(0.4, 0.6, (B, T)).astype(np.float32)
    if B * T >= 14:
        assert c.raw.min() < 0 and c.raw.max() > 1
    c.len = rng.integers(1, T + 1, B).astype(np.int32)
    for i, v in enumerate([T, 1, 0, T + 3][:B]):
        c.len[i] = v
    c.glast = rng.normal(0, 1, (B, U)).astype(np.float32)
    # the masked scores as the kernels read them: float32 values, the same in every precision
    c.scores = mask_scores_t(_t(c.raw, F64), c.len, norm).numpy().astype(np.float32)
    return c


def augru_grads(c, dt=F64, pre=None):
    """(last, dx, ds_raw, da, dW, dU) of sum(last * glast).  The AUGRU reads
    the float32 scores c.scores; the mask's backward is taken at them."""
    x, W, U = (_t(v, dt).requires_grad_() for v in (c.x, c.W, c.Ur))
    a = _t(c.scores, dt).requires_grad_()
    last = augru_t(x, a, W, U, c.update, pre)
    dx, da, dW, dU = torch.autograd.grad((last * _t(c.glast, dt)).sum(), (x, a, W, U))
    # ds: through the mask / softmax at p = the scores
    valid = (torch.arange(c.T)[None] < _t(c.len, torch.int64).reshape(-1, 1)).to(dt)
    if c.norm:
        p = a.detach() * valid
        ds = p * (da - (p * da).sum(1, keepdim=True))
    else:
        ds = da * valid
    return [v.detach().numpy() for v in (last, dx, ds, da, dW, dU)]


@functools.lru_cache(maxsize=None)
def augru_case(*k):
    c = _augru_inputs(*k)
    c.pre = []
    c.ref = augru_grads(c, pre=c.pre)
    return c


# ------------------------------------------------------------------ CPU
def test_restatement_forward_matches_the_inference_reference():
    """gru_t / augru_t against tests.test_dien's numpy gru_ref / augru_ref."""
    c = gru_case(5, 7, 8, 12)
    np.testing.assert_allclose(c.ref["both"][0], gru_ref(c.x, c.W, c.Ur, c.b), rtol=1e-12, atol=1e-14)
    for k in ((5, 7, 8, 12, True, "reference", 1.0, 0), (33, 7, 12, 12, False, "paper", 1.0, 0)):
        a = augru_case(*k)
        np.testing.assert_allclose(a.ref[0], augru_ref(a.x, a.scores, a.W, a.Ur, a.update), rtol=1e-12, atol=1e-14)


def _fd(f, arrs, step=1e-6):
    """Central differences of the scalar f(*arrs) in float64, every element."""
    out = []
    for i, a in enumerate(arrs):
        g = np.zeros_like(a)
        it = np.nditer(a, flags=["multi_index"])
        for _ in it:
            j = it.multi_index
            hi, lo = [v.copy() for v in arrs], [v.copy() for v in arrs]
            hi[i][j] += step
            lo[i][j] -= step
            g[j] = (f(*hi) - f(*lo)) / (2 * step)
        out.append(g)
    return out


def test_gru_gradients_match_finite_differences():
    c = _gru_inputs(3, 4, 3, 2)
    _, dx, dW, dU, db = gru_grads(c, "both")

    def f(x, W, U, b):
        seq = gru_t(*(_t(v, F64) for v in (x, W, U, b)))
        return float((seq * _t(c.gseq, F64)).sum() + (seq[:, -1] * _t(c.glast, F64)).sum())

    for name, got, want in zip("x W U b".split(), (dx, dW, dU, db),
                               _fd(f, [np.asarray(v, np.float64) for v in (c.x, c.W, c.Ur, c.b)])):
        assert np.max(np.abs(got - want)) <= 1e-6 * max(1.0, np.max(np.abs(want))), name


@pytest.mark.parametrize("norm", [True, False])
@pytest.mark.parametrize("update", ["reference", "paper"])
def test_augru_gradients_match_finite_differences(norm, update):
    """x, W, U and the RAW scores (through mask and softmax): the float64
    softmax of the raw scores stands in for the float32 scores the GPU reads."""
    c = _augru_inputs(4, 4, 3, 2, norm, update, 1.0)
    c.scores = mask_scores_t(_t(c.raw, F64), c.len, norm).numpy()  # float64: differentiable in raw
    _, dx, ds, _, dW, dU = augru_grads(c)
    pre = []
    augru_t(_t(c.x, F64), _t(c.scores, F64), _t(c.W, F64), _t(c.Ur, F64), update, pre)
    assert min(np.min(np.abs(np.abs(v) - 2.5)) for p in pre for v in p) > 1e-3

    def f(x, raw, W, U):
        s = mask_scores_t(_t(raw, F64), c.len, norm)
        return float((augru_t(_t(x, F64), s, _t(W, F64), _t(U, F64), update) * _t(c.glast, F64)).sum())

    for name, got, want in zip("x raw W U".split(), (dx, ds, dW, dU),
                               _fd(f, [np.asarray(v, np.float64) for v in (c.x, c.raw, c.W, c.Ur)])):
        assert np.max(np.abs(got - want)) <= 1e-6 * max(1.0, np.max(np.abs(want))), name
    assert np.all(ds[np.arange(4)[None] >= c.len[:, None]] == 0)


def test_gru_backward_step_by_hand():
    """U 1, one step from h = 0: x = 1, W = [1, 2, 0.5], bias rows [0, 0, 0] /
    [0, 0, 3], dh = 1.  z = sig(1), r = sig(2), hr_h = 3, hh = tanh(0.5 + 3 r),
    h = (1 - z) hh.  dz = -hh, dhh = 1 - z, dc = dhh (1 - hh^2), da_z = dz z
    (1 - z), dr = 3 dc, da_r = dr r (1 - r); dx = gx . W, dbias[1] = [da_z,
    da_r, dc r]; dU multiplies h_prev = 0."""
    sig = lambda v: 1 / (1 + np.exp(-v))
    c = Case()
    c.x, c.W, c.Ur = np.array([[[1.0]]]), np.array([[1.0, 2.0, 0.5]]), np.array([[0.3, -0.2, 0.7]])
    c.b = np.array([[0.0, 0, 0], [0, 0, 3.0]])
    c.gseq, c.glast = np.zeros((1, 1, 1)), np.ones((1, 1))
    seq, dx, dW, dU, db = gru_grads(c, "last")
    z, r = sig(1.0), sig(2.0)
    hh = np.tanh(0.5 + 3 * r)
    dc = (1 - z) * (1 - hh ** 2)
    gx = np.array([-hh * z * (1 - z), 3 * dc * r * (1 - r), dc])
    np.testing.assert_allclose(seq[0, 0, 0], (1 - z) * hh, rtol=1e-14)
    np.testing.assert_allclose(dW[0], gx, rtol=1e-13)
    np.testing.assert_allclose(dx[0, 0, 0], gx @ c.W[0], rtol=1e-13)
    np.testing.assert_allclose(db, [gx, gx * [1, 1, r]], rtol=1e-13)
    assert np.all(dU == 0)


def test_augru_backward_step_by_hand():
    """U 1, two steps, score 0.5 at both, W = [2, 1, 0.5], U = [1, 1, 1], x =
    [1, 1], dlast = 1.  Step 1 from h = 0: u1 = hsig(2) = 0.9, h1 = (1 - 0.45)
    tanh(0.5).  Step 2: a_z = 2 + h1, u2 = 0.9 + 0.2 h1, z2 = 0.5 u2, a_r = 1 +
    h1, r2 = 0.7 + 0.2 h1, c = 0.5 + r2 h1, hh2 = tanh(c).  Backward at step 2
    (reference blend): dz = h1 - hh2, keep = z2, dhh = 1 - z2, dc = dhh (1 -
    hh2^2), d(rh) = dc, dr = dc h1, da_2 = dz u2, da_z = dz 0.5 0.2, da_r = dr
    0.2, dh1 = keep + d(rh) r2 + da_z + da_r."""
    c = Case()
    c.T, c.norm, c.update, c.len = 2, False, "reference", np.array([2])
    c.x, c.W, c.Ur = np.array([[[1.0], [1.0]]]), np.array([[2.0, 1.0, 0.5]]), np.array([[1.0, 1.0, 1.0]])
    c.scores, c.glast = np.array([[0.5, 0.5]]), np.ones((1, 1))
    last, dx, ds, da, dW, dU = augru_grads(c)
    hh1 = np.tanh(0.5)
    h1 = 0.55 * hh1
    u2, r2 = 0.9 + 0.2 * h1, 0.7 + 0.2 * h1
    z2, hh2 = 0.5 * u2, np.tanh(0.5 + r2 * h1)
    np.testing.assert_allclose(last[0, 0], z2 * h1 + (1 - z2) * hh2, rtol=1e-14)
    dz = h1 - hh2
    dc = (1 - z2) * (1 - hh2 ** 2)
    daz, dar = dz * 0.5 * 0.2, dc * h1 * 0.2
    dh1 = z2 + dc * r2 + daz + dar
    np.testing.assert_allclose(da[0, 1], dz * u2, rtol=1e-13)
    np.testing.assert_allclose(dx[0, 1, 0], np.array([daz, dar, dc]) @ c.W[0], rtol=1e-13)
    # step 1 (h_prev = 0): dz = -hh1 dh1, dhh = 0.55 dh1; u1 = 0.9 inside the linear range
    np.testing.assert_allclose(da[0, 0], -hh1 * dh1 * 0.9, rtol=1e-13)
    dc1 = 0.55 * dh1 * (1 - hh1 ** 2)
    np.testing.assert_allclose(dW[0], [daz + -hh1 * dh1 * 0.5 * 0.2, dar, dc + dc1], rtol=1e-13)
    np.testing.assert_allclose(dU[0], [daz * h1, dar * h1, dc * r2 * h1], rtol=1e-13)
    np.testing.assert_array_equal(ds, da)


@pytest.mark.parametrize("k", GRU_SHAPES, ids=_aid)
def test_gru_cases_are_well_conditioned(k):
    c = gru_case(*k)
    for mode in GRU_MODES:
        got = gru_grads(c, mode, torch.float32)
        for name, g, r in zip("seq dx dW dU db".split(), got, c.ref[mode]):
            e = scaled_err(g, r)
            print(f"{_aid(k)} {mode} {name}: float32 scaled error {e:.2e}")
            assert e <= RTOL / 4, f"{mode} {name}: {e:.2e}"


@pytest.mark.parametrize("k", AUGRU_CASES, ids=_aid)
def test_augru_cases_are_well_conditioned(k):
    c = augru_case(*k)
    got = augru_grads(c, torch.float32)
    for name, g, r in zip("last dx ds da dW dU".split(), got, c.ref):
        e = scaled_err(g, r)
        print(f"{_aid(k)} {name}: float32 scaled error {e:.2e}")
        assert e <= RTOL / 4, f"{name}: {e:.2e}"


@pytest.mark.parametrize("k", AUGRU_CASES, ids=_aid)
def test_augru_cases_stay_off_the_kinks(k):
    """No gate pre-activation within 1e-3 of +-2.5 (the float32 one is off by
    about 1e-6 of a value near 3); the saturating cases put at least 5 % of the
    z and of the r pre-activations beyond each of +2.5 and -2.5."""
    c = augru_case(*k)
    az = np.stack([p[0] for p in c.pre])
    ar = np.stack([p[1] for p in c.pre])
    for v in (az, ar):
        assert np.min(np.abs(np.abs(v) - 2.5)) > 1e-3
    if k in SATURATING:
        for name, v in (("z", az), ("r", ar)):
            hi, lo = float(np.mean(v > 2.5)), float(np.mean(v < -2.5))
            print(f"{_aid(k)} {name}: {hi:.3f} above 2.5, {lo:.3f} below -2.5")
            assert hi >= 0.05 and lo >= 0.05, name


def test_size_queries():
    lib = _lib.lib()
    up = lambda v: (v + 15) // 16 * 16
    for T, din, u, B in [(1, 16, 16, 1), (7, 8, 12, 5), (50, 36, 36, 4096), (5, 64, 64, 16), (3, 5, 17, 0)]:
        assert lib.rs_gru_saved_size(T, din, u, B) == B * T * 5 * up(u)
        assert lib.rs_augru_saved_size(T, din, u, B) == B * T * 4 * up(u)
    for u in (1, 12, 16, 17, 36, 64):
        assert lib.rs_gru_bwd_prepared_size(u) == 3 * up(u) * up(u)
    assert lib.rs_gru_saved_size(0, 12, 12, 3) == -1 and b"rs_gru_saved_size" in lib.rs_last_error_string()
    assert lib.rs_gru_saved_size(7, 65, 12, 3) == -1 and lib.rs_gru_saved_size(7, 12, 65, 3) == -1
    assert lib.rs_gru_saved_size(7, 12, 12, -1) == -1
    assert lib.rs_augru_saved_size(0, 12, 12, 3) == -1 and b"rs_augru_saved_size" in lib.rs_last_error_string()
    assert lib.rs_augru_saved_size(7, 12, 0, 3) == -1
    assert lib.rs_gru_bwd_prepared_size(65) == -1 and lib.rs_gru_bwd_prepared_size(0) == -1
    assert b"rs_gru_bwd_prepared_size" in lib.rs_last_error_string()


def test_argument_validation_returns_an_error_code():
    """Refusals come back before any device work (16 stands for 'an aligned
    pointer that is not null'; it is never dereferenced)."""
    lib = _lib.lib()
    p = C.c_void_p(16)
    names = {
        "rs_gru_train_fwd": ("x xb xt T din U prep seq last ls saved B st",
                             dict(x=p, xb=35, xt=5, T=7, din=5, U=9, prep=p, seq=p, last=None, ls=0, saved=p, B=3,
                                  st=None)),
        "rs_augru_train_fwd": ("x xb xt sc ss T din U upd prep last ls saved B st",
                               dict(x=p, xb=35, xt=5, sc=p, ss=7, T=7, din=5, U=9, upd=0, prep=p, last=p, ls=9, saved=p,
                                    B=3, st=None)),
        "rs_gru_bwd": ("saved dseq dlast dls T U prep gx gh hp B st",
                       dict(saved=p, dseq=p, dlast=p, dls=9, T=7, U=9, prep=p, gx=p, gh=p, hp=p, B=3, st=None)),
        "rs_augru_bwd": ("saved sc ss len lk norm dlast dls T U upd prep gx hrh ds da B st",
                         dict(saved=p, sc=p, ss=7, len=p, lk=0, norm=1, dlast=p, dls=9, T=7, U=9, upd=0, prep=p, gx=p,
                              hrh=p, ds=p, da=None, B=3, st=None)),
    }
    bad = {
        "rs_gru_train_fwd": [dict(x=None), dict(prep=None), dict(saved=None), dict(seq=None, last=None), dict(saved=C.c_void_p(4)), dict(T=0),
                             dict(din=65), dict(U=65), dict(U=0), dict(xt=4), dict(xb=34), dict(B=-1)],
        "rs_augru_train_fwd": [dict(x=None), dict(sc=None), dict(last=None), dict(saved=None), dict(prep=None),
                               dict(T=0), dict(din=65), dict(U=65), dict(ss=6), dict(ls=8), dict(upd=2)],
        "rs_gru_bwd": [dict(saved=None), dict(prep=None), dict(dseq=None, dlast=None), dict(dls=8), dict(T=0),
                       dict(U=65), dict(U=0), dict(gx=None), dict(gh=None), dict(hp=None), dict(B=-1),
                       dict(saved=C.c_void_p(8))],
        "rs_augru_bwd": [dict(saved=None), dict(sc=None), dict(len=None), dict(dlast=None), dict(prep=None),
                         dict(ss=6), dict(dls=8), dict(lk=2), dict(T=0), dict(U=65), dict(upd=2), dict(gx=None),
                         dict(hrh=None), dict(ds=None), dict(B=-1)],
    }
    for name, (order, base) in names.items():
        fn = getattr(lib, name)
        run = lambda **k: fn(*[{**base, **k}[a] for a in order.split()])
        assert run(B=0) == 0, name                                   # empty batch: nothing launched
        for k in bad[name]:
            assert run(**k) == -1, (name, k)
            assert name.encode() in lib.rs_last_error_string(), (name, k)
    assert lib.rs_gru_bwd(p, None, p, 9, 7, 9, p, p, p, p, 0, None) == 0
    assert lib.rs_gru_prepare_bwd(9, None, p, None) == -1 and lib.rs_gru_prepare_bwd(9, p, None, None) == -1
    assert lib.rs_gru_prepare_bwd(65, p, p, None) == -1 and b"rs_gru_prepare_bwd" in lib.rs_last_error_string()


# ------------------------------------------------------------------ GPU
def _dev(a, gpu):
    return torch.as_tensor(np.ascontiguousarray(a)).to(gpu)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _prepared(gpu, din, U, W, Ur, b):
    lib = _lib.lib()
    prep = torch.empty(lib.rs_gru_prepared_size(din, U), device=gpu)
    pb = torch.empty(lib.rs_gru_bwd_prepared_size(U), device=gpu)
    Wd, Ud, bd = _dev(W, gpu), _dev(Ur, gpu), (None if b is None else _dev(b, gpu))
    _lib.call("rs_gru_prepare", din, U, _lib.ptr(Wd), _lib.ptr(Ud), _lib.ptr(bd), _lib.ptr(prep), _stream())
    _lib.call("rs_gru_prepare_bwd", U, _lib.ptr(Ud), _lib.ptr(pb), _stream())
    return prep, pb


def run_gru(gpu, c, mode, fill, rows=slice(None)):
    """The entries on buffers pre-filled with ``fill``: every output as numpy."""
    p, call = _lib.ptr, _lib.call
    x = _dev(c.x[rows], gpu)
    B, T, din, U = x.shape[0], c.T, c.din, c.U
    prep, pb = _prepared(gpu, din, U, c.W, c.Ur, c.b)
    full = lambda *s: torch.full(s, fill, dtype=torch.float32, device=gpu)
    saved = full(_lib.lib().rs_gru_saved_size(T, din, U, B))
    seq, last = full(B, T, U), full(B, U)
    call("rs_gru_train_fwd", p(x), x.stride(0), x.stride(1), T, din, U, p(prep), p(seq), p(last), U, p(saved), B,
         _stream())
    seq0, last0 = full(B, T, U), full(B, U)
    call("rs_gru_fwd", p(x), x.stride(0), x.stride(1), T, din, U, p(prep), p(seq0), p(last0), U, B, _stream())
    dseq = _dev(c.gseq[rows], gpu) if mode in ("seq", "both") else None
    dlast = _dev(c.glast[rows], gpu) if mode in ("last", "both") else None
    gx, gh, hp = full(B * T, 3 * U), full(B * T, 3 * U), full(B * T, U)
    call("rs_gru_bwd", p(saved), p(dseq), p(dlast), U, T, U, p(pb), p(gx), p(gh), p(hp), B, _stream())
    out = dict(seq=seq, last=last, seq0=seq0, last0=last0, saved=saved, gx=gx, gh=gh, hp=hp)
    return {k: v.cpu().numpy() for k, v in out.items()}


@gpu_test
@pytest.mark.parametrize("mode", GRU_MODES)
@pytest.mark.parametrize("k", GRU_SHAPES, ids=_aid)
def test_gru_backward(gpu, k, mode):
    c = gru_case(*k)
    seq_r, dx_r, dW_r, dU_r, db_r = c.ref[mode]
    g = rs.GRU(c.U, return_sequences=True, device=gpu, seed=0, input_dim=c.din)
    g.set_keras_weights({"kernel": c.W, "recurrent_kernel": c.Ur, "bias": c.b})
    x = _dev(c.x, gpu)
    seq, saved = g.train_forward(x)
    assert torch.equal(seq, g(x))                                     # the inference launch's bits
    assert_scaled_close(seq, seq_r, what="seq")
    dx, dW, dU, db = g.backward(x, saved, dseq=_dev(c.gseq, gpu) if mode != "last" else None,
                                dlast=_dev(c.glast, gpu) if mode != "seq" else None)
    for name, got, want in (("dx", dx, dx_r), ("dW", dW, dW_r), ("dU", dU, dU_r), ("dbias", db, db_r)):
        assert_scaled_close(got, want, what=f"GRU {mode} {name}")
    assert g.backward(x, saved, dlast=_dev(c.glast, gpu), d_in=False)[0] is None


@gpu_test
@pytest.mark.parametrize("k", [(17, 2, 12, 12), (33, 7, 12, 12), (5, 7, 20, 12), (16, 5, 64, 64)], ids=_aid)
def test_gru_entries_write_everything_and_split_bitwise(gpu, k):
    c = gru_case(*k)
    a = run_gru(gpu, c, "both", float("nan"))
    for name, v in a.items():
        assert np.isfinite(v).all(), name                             # every element written
    assert np.array_equal(a["seq"], a["seq0"]) and np.array_equal(a["last"], a["last0"])
    b = run_gru(gpu, c, "both", 3.0)
    for name in a:
        assert np.array_equal(a[name], b[name]), name                 # nothing read before it is written
    if c.B > 1:
        cut = min(16, c.B - 1) if c.B != 33 else 17
        lo, hi = run_gru(gpu, c, "both", 0.0, slice(0, cut)), run_gru(gpu, c, "both", 0.0, slice(cut, None))
        for name in ("seq", "last", "gx", "gh", "hp"):
            assert np.array_equal(np.concatenate([lo[name], hi[name]]), a[name]), name
    assert np.all(a["hp"].reshape(c.B, c.T, c.U)[:, 0] == 0)           # h_prev of step 0: a zero row


def run_augru(gpu, c, fill, rows=slice(None), want_da=True, len_dtype=np.int32):
    p, call = _lib.ptr, _lib.call
    x, sc, L = _dev(c.x[rows], gpu), _dev(c.scores[rows], gpu), _dev(c.len[rows].astype(len_dtype), gpu)
    B, T, din, U = x.shape[0], c.T, c.din, c.U
    upd = {"reference": 0, "paper": 1}[c.update]
    prep, pb = _prepared(gpu, din, U, c.W, c.Ur, None)
    full = lambda *s: torch.full(s, fill, dtype=torch.float32, device=gpu)
    saved = full(_lib.lib().rs_augru_saved_size(T, din, U, B))
    last, last0 = full(B, U), full(B, U)
    call("rs_augru_train_fwd", p(x), x.stride(0), x.stride(1), p(sc), T, T, din, U, upd, p(prep), p(last), U, p(saved),
         B, _stream())
    call("rs_augru_fwd", p(x), x.stride(0), x.stride(1), p(sc), T, T, din, U, upd, p(prep), p(last0), U, B, _stream())
    dlast = _dev(c.glast[rows], gpu)
    gx, hrh, ds = full(B * T, 3 * U), full(B * T, 2 * U), full(B, T)
    da = full(B, T) if want_da else None
    call("rs_augru_bwd", p(saved), p(sc), T, p(L), _lib.id_kind(L), int(c.norm), p(dlast), U, T, U, upd, p(pb), p(gx),
         p(hrh), p(ds), p(da), B, _stream())
    out = dict(last=last, last0=last0, saved=saved, gx=gx, hrh=hrh, ds=ds)
    if want_da:
        out["da"] = da
    return {k: v.cpu().numpy() for k, v in out.items()}


@gpu_test
@pytest.mark.parametrize("k", AUGRU_CASES, ids=_aid)
def test_augru_backward(gpu, k):
    c = augru_case(*k)
    last_r, dx_r, ds_r, da_r, dW_r, dU_r = c.ref
    au = rs.AUGRU(c.U, augru_update=c.update, device=gpu, seed=0, input_dim=c.din)
    au.set_keras_weights({"kernel": c.W, "recurrent_kernel": c.Ur})
    x, sc = _dev(c.x, gpu), _dev(c.scores, gpu)
    last, saved = au.train_forward(x, sc)
    assert torch.equal(last, au(x, sc))
    assert_scaled_close(last, last_r, what="last")
    dx, ds, da, dW, dU = au.backward(x, sc, c.len, saved, _dev(c.glast, gpu), weight_normalization=c.norm,
                                     want_da=True)
    for name, got, want in (("dx", dx, dx_r), ("ds", ds, ds_r), ("da", da, da_r), ("dW", dW, dW_r), ("dU", dU, dU_r)):
        assert_scaled_close(got, want, what=f"AUGRU {name}")
    masked = np.arange(c.T)[None] >= c.len[:, None]
    assert np.all(ds.cpu().numpy()[masked] == 0)                      # exactly 0 at t >= len
    assert au.backward(x, sc, c.len, saved, _dev(c.glast, gpu), weight_normalization=c.norm)[2] is None


@gpu_test
@pytest.mark.parametrize("k", [(17, 2, 12, 12, True, "reference", 1.0, 0), (33, 7, 12, 12, False, "paper", 1.0, 0),
                               (5, 7, 20, 12, True, "reference", 1.0, 0), (16, 5, 64, 64, False, "reference", 1.0, 0)],
                         ids=_aid)
def test_augru_entries_write_everything_and_split_bitwise(gpu, k):
    c = augru_case(*k)
    a = run_augru(gpu, c, float("nan"))
    for name, v in a.items():
        assert np.isfinite(v).all(), name
    assert np.array_equal(a["last"], a["last0"])
    b = run_augru(gpu, c, 3.0, want_da=False, len_dtype=np.int64)
    for name in b:
        assert np.array_equal(a[name], b[name]), name
    cut = min(16, c.B - 1) if c.B != 33 else 17
    lo, hi = run_augru(gpu, c, 0.0, slice(0, cut)), run_augru(gpu, c, 0.0, slice(cut, None))
    for name in ("last", "gx", "hrh", "ds", "da"):
        assert np.array_equal(np.concatenate([lo[name], hi[name]]), a[name]), name
    masked = np.arange(c.T)[None] >= c.len[:, None]
    assert np.all(a["ds"][masked] == 0)
    if c.B > 2:
        assert np.all(a["ds"][2] == 0)                                # len 0: a zero row


@gpu_test
def test_layer_backward_is_deterministic_and_capturable(gpu):
    """The whole GRU backward (chain launch, gemms, column sums) twice: the
    same bits; and once under stream capture."""
    c = gru_case(33, 7, 12, 12)
    g = rs.GRU(c.U, return_sequences=True, device=gpu, seed=0, input_dim=c.din)
    g.set_keras_weights({"kernel": c.W, "recurrent_kernel": c.Ur, "bias": c.b})
    x, dseq, dlast = _dev(c.x, gpu), _dev(c.gseq, gpu), _dev(c.glast, gpu)
    _, saved = g.train_forward(x)
    first = g.backward(x, saved, dseq, dlast)
    for a, b in zip(first, g.backward(x, saved, dseq, dlast)):
        assert torch.equal(a, b)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        g.backward(x, g.train_forward(x)[1], dseq, dlast)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = g.backward(x, g.train_forward(x)[1], dseq, dlast)
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(first, got):
        assert torch.equal(a, b)


@gpu_test
def test_dx_bits_do_not_depend_on_the_batch(gpu):
    """dx = gx W^T of a sample from GRU.backward / AUGRU.backward, bit for bit,
    in a batch of 4400 (B T = 22,000 rows: 344 output tiles, where rs_gemm with
    a workspace would cut K = 192 into 2 slices), in its first 16 samples alone
    (80 rows: 2 tiles, 3 slices) and in a 17 / rest split."""
    rng = np.random.default_rng(5)
    B, T, U = 4400, 5, 64
    w = rand_evolution_weights(rng, U, (), "relu")
    x = _dev(rng.normal(0, 0.5, (B, T, U)).astype(np.float32), gpu)
    gs, gl = (_dev(rng.normal(0, 1, s).astype(np.float32), gpu) for s in ((B, T, U), (B, U)))
    sc = _dev(rng.uniform(0, 1, (B, T)).astype(np.float32), gpu)
    L = _dev(rng.integers(0, T + 2, B).astype(np.int32), gpu)
    g = rs.GRU(U, return_sequences=True, device=gpu, seed=0, input_dim=U)
    g.set_keras_weights({"kernel": w["gru1/kernel"], "recurrent_kernel": w["gru1/recurrent_kernel"],
                         "bias": w["gru1/bias"]})
    au = rs.AUGRU(U, device=gpu, seed=0, input_dim=U)
    au.set_keras_weights({"kernel": w["gru2/kernel"], "recurrent_kernel": w["gru2/recurrent_kernel"]})

    def gru_dx(r):
        return g.backward(x[r], g.train_forward(x[r])[1], gs[r], gl[r])[0]

    def augru_out(r):
        out = au.backward(x[r], sc[r], L[r], au.train_forward(x[r], sc[r])[1], gl[r], True, want_da=True)
        return out[:3]                                                  # dx, ds, da

    whole, lo, hi = slice(None), slice(0, 17), slice(17, None)
    full = gru_dx(whole)
    assert torch.equal(gru_dx(slice(0, 16)), full[:16])
    assert torch.equal(torch.cat([gru_dx(lo), gru_dx(hi)]), full)
    full = augru_out(whole)
    for a, b, c, d in zip(full, augru_out(slice(0, 16)), augru_out(lo), augru_out(hi)):
        assert torch.equal(b, a[:16]) and torch.equal(torch.cat([c, d]), a)


EVO_CASES = [dict(B=33, T=7, D=12, act="dice", norm=True, att=(64, 16), update="reference"),
             dict(B=17, T=5, D=20, act="sigmoid", norm=False, att=(16, 8), update="paper")]
_eid = lambda k: "-".join(str(v) for v in k.values()).replace(" ", "")
ATT_P = "attention_sequence_pooling_layer/local_att/"


def _evo_inputs(k):
    rng = np.random.default_rng([7, k["B"], k["T"], k["D"], k.get("seed", 0)])
    c = Case()
    c.w = rand_evolution_weights(rng, k["D"], k["att"], k["act"])
    c.keys = rng.normal(0, 0.5, (k["B"], k["T"], k["D"])).astype(np.float32)
    c.q = rng.normal(0, 0.5, (k["B"], k["D"])).astype(np.float32)
    c.len = rng.integers(1, k["T"] + 1, k["B"]).astype(np.int32)
    c.len[:4] = [k["T"], 1, 0, k["T"] + 3]
    c.ghist = rng.normal(0, 1, (k["B"], k["D"])).astype(np.float32)
    c.gh1 = rng.normal(0, 0.3, (k["B"], k["T"], k["D"])).astype(np.float32)
    return c


def evo_grads(k, c, dt=F64):
    """InterestEvolution in training mode: (hist, H1, dkeys, dq, {weight: gradient},
    moved statistics) of sum(hist * ghist) + sum(H1 * gh1)."""
    tw = {n: _t(v, dt).requires_grad_(not n.endswith(STATS)) for n, v in c.w.items()}
    keys, q = _t(c.keys, dt).requires_grad_(), _t(c.q, dt).requires_grad_()
    B, T, D = keys.shape
    moved = {}
    H1 = gru_t(keys, tw["gru1/kernel"], tw["gru1/recurrent_kernel"], tw["gru1/bias"])
    Q = q[:, None].expand(B, T, D)
    e = torch.cat([Q, H1, Q - H1, Q * H1], -1).reshape(B * T, 4 * D)
    for i in range(len(k["att"])):
        e = e @ tw[ATT_P + f"dnn/kernel{i}"] + tw[ATT_P + f"dnn/bias{i}"]
        e = _dice_train(e, tw, ATT_P + f"dnn/dice{i}/", moved) if k["act"] == "dice" else torch.sigmoid(e)
    s = mask_scores_t((e @ tw[ATT_P + "kernel"] + tw[ATT_P + "bias"]).reshape(B, T), c.len, k["norm"])
    hist = augru_t(H1, s, tw["gru2/kernel"], tw["gru2/recurrent_kernel"], k["update"])
    train = [n for n, v in tw.items() if v.requires_grad]
    loss = (hist * _t(c.ghist, dt)).sum() + (H1 * _t(c.gh1, dt)).sum()
    g = torch.autograd.grad(loss, [keys, q] + [tw[n] for n in train])
    return (hist.detach().numpy(), H1.detach().numpy(), g[0].numpy(), g[1].numpy(),
            {n: v.numpy() for n, v in zip(train, g[2:])}, {n: v.numpy() for n, v in moved.items()})


def _evo_compared(c, out):
    """What the layer test compares, from evo_grads' (or the layer's) results:
    hist, H1 and dkeys as they are; q and every weight after an SGD step of LR,
    the measure of the model tests.  Under the softmax sum_t ds_t = 0, so dq and
    the attention unit's gradients are differences of nearly equal sums with no
    scale of their own (the score bias's gradient is exactly 0): their scale is
    the step they make."""
    hist, h1, dkeys, dq, grads, moved = out
    step = lambda w, g: np.asarray(w, np.float64) - LR * np.asarray(g, np.float64).reshape(np.shape(w))
    res = {"hist": hist, "H1": h1, "dkeys": dkeys, "q after a step": step(c.q, dq)}
    res.update({n + " after a step": step(c.w[n], g) for n, g in grads.items()})
    res.update(moved)
    return res


@pytest.mark.parametrize("k", EVO_CASES, ids=_eid)
def test_evolution_cases_are_well_conditioned(k):
    c = _evo_inputs(k)
    ref, got = _evo_compared(c, evo_grads(k, c)), _evo_compared(c, evo_grads(k, c, torch.float32))
    for name in ref:
        e = scaled_err(got[name], ref[name])
        assert e <= RTOL / 4, f"{name}: {e:.2e}"


@gpu_test
@pytest.mark.parametrize("k", EVO_CASES, ids=_eid)
def test_interest_evolution_trains_on_its_own(gpu, k):
    """InterestEvolution.train_forward / train_backward against the restatement:
    hist, H1, dkeys, dq, every weight's gradient and the moved Dice statistics;
    hist equals the inference forward's where no batch statistics enter."""
    c = _evo_inputs(k)
    hist_r, h1_r, dkeys_r, dq_r, grads_r, moved_r = evo_grads(k, c)
    m = rs.InterestEvolution(k["D"], k["att"], k["act"], k["norm"], augru_update=k["update"], device=gpu, seed=0)
    m.set_keras_weights(c.w)
    keys, q = _dev(c.keys, gpu), _dev(c.q, gpu)
    if k["act"] != "dice":
        want = m.forward_unfused(keys, q, c.len).clone()
    hist, H1, ctx = m.train_forward(keys, q, c.len)
    if k["act"] != "dice":
        assert torch.equal(hist, want)
    dkeys, dq, updates = m.train_backward(ctx, _dev(c.ghist, gpu), dh1=_dev(c.gh1, gpu))
    names = {id(p): n for n, p in m.keras_weights().items()}
    grads = {names[id(w)]: g.cpu().numpy() for w, g, _ in updates}
    assert sorted(grads) == sorted(grads_r)
    kw = m.keras_weights()
    moved = {n: kw[n].cpu().numpy() for n in moved_r}
    got = _evo_compared(c, (hist.cpu().numpy(), H1.cpu().numpy(), dkeys.cpu().numpy(), dq.cpu().numpy(), grads, moved))
    for name, want in _evo_compared(c, (hist_r, h1_r, dkeys_r, dq_r, grads_r, moved_r)).items():
        assert_scaled_close(got[name], want, what=name)
    for n, v in c.w.items():                                            # nothing but the statistics moved
        if not n.endswith(STATS):
            assert torch.equal(kw[n].cpu(), torch.as_tensor(v).reshape(kw[n].shape)), n


# =================================================================== the model
ATT = "attention_sequence_pooling_layer/local_att/"
HIST = ["item_id", "cate_id"]
MODEL_CFGS = {
    "defaults": dict(),
    "negsampling": dict(use_negsampling=True, alpha=0.7, att_activation="sigmoid", att_weight_normalization=False),
    "bn-dice-paper": dict(att_hidden_units=(32, 16, 8), att_activation="relu", use_bn=True, dnn_activation="dice",
                          augru_update="paper"),
    "l2-dropout": dict(l2_reg_dnn=1e-3, l2_reg_embedding=1e-3, dnn_dropout=0.5),
}
MODEL_CASES = [(d, c) for d in ("toy", "wide") for c in MODEL_CFGS]


def toy_data(neg):
    """The reference's get_xy_fd (model/dien.py:172-213): B 3, T 4."""
    x = {"user": np.array([0, 1, 2]), "gender": np.array([0, 1, 0]), "item_id": np.array([1, 2, 3]),
         "cate_id": np.array([1, 2, 2]), "pay_score": np.array([0.1, 0.2, 0.3], np.float32),
         "hist_item_id": np.array([[1, 2, 3, 0], [1, 2, 3, 0], [1, 2, 0, 0]]),
         "hist_cate_id": np.array([[1, 2, 2, 0], [1, 2, 2, 0], [1, 2, 0, 0]]), "seq_length": np.array([3, 3, 2])}
    if neg:
        x["neg_hist_item_id"], x["neg_hist_cate_id"] = x["hist_item_id"].copy(), x["hist_cate_id"].copy()
    return toy_columns(neg), x, np.array([1.0, 0.0, 1.0], np.float32)


def wide_data(neg):
    """B 37, T 7, widths (8, 4), vocabularies small enough that rows repeat, a
    dense feature and a pooled 'mean' column; lengths 0, 1, T and past T."""
    S, V = rs.SparseFeat, rs.VarLenSparseFeat
    B, T = 37, 7
    cols = [S("user", 5, embedding_dim=6), S("item_id", 6, embedding_dim=8), S("cate_id", 4, embedding_dim=4),
            rs.DenseFeat("price", 1),
            V(S("hist_item_id", 6, embedding_dim=8, embedding_name="item_id"), maxlen=T, length_name="seq_length"),
            V(S("hist_cate_id", 4, embedding_dim=4, embedding_name="cate_id"), maxlen=T, length_name="seq_length"),
            V(S("tags", 5, embedding_dim=3), maxlen=4, combiner="mean", length_name="tag_len")]
    if neg:
        cols += [V(S("neg_hist_item_id", 6, embedding_dim=8, embedding_name="item_id"), maxlen=T,
                   length_name="seq_length"),
                 V(S("neg_hist_cate_id", 4, embedding_dim=4, embedding_name="cate_id"), maxlen=T,
                   length_name="seq_length")]
    rng = np.random.default_rng(41)
    x = {"user": rng.integers(0, 5, B), "item_id": rng.integers(0, 6, B), "cate_id": rng.integers(0, 4, B),
         "price": rng.normal(0, 1, B).astype(np.float32), "hist_item_id": rng.integers(0, 6, (B, T)),
         "hist_cate_id": rng.integers(0, 4, (B, T)), "tags": rng.integers(0, 5, (B, 4)),
         "seq_length": rng.integers(1, T + 1, B), "tag_len": rng.integers(0, 5, B)}
    x["seq_length"][:4] = [T, 1, 0, T + 3]
    if neg:
        x["neg_hist_item_id"], x["neg_hist_cate_id"] = rng.integers(0, 6, (B, T)), rng.integers(0, 4, (B, T))
    return cols, x, rng.integers(0, 2, B).astype(np.float32)


def make_model(data, cfg, device):
    kw = MODEL_CFGS[cfg]
    cols, x, y = (toy_data if data == "toy" else wide_data)(bool(kw.get("use_negsampling")))
    m = rs.DIEN(cols, HIST, dnn_hidden_units=(8, 4), device=device, seed=11, **kw)
    return m, x, y


def rand_weights(named, rng, att_scale=1.0):
    """Random Keras-named weights.  ``att_scale`` widens the attention unit's
    hidden kernels and biases: with relu there, 3 steps of B T (32 + 16 + 8)
    pre-activations of unit scale cannot all stay 1e-4 away from 0."""
    w = {}
    for k, p in named.items():
        s = tuple(p.shape)
        if k.endswith("moving_variance"):
            v = rng.uniform(0.5, 1.5, s)
        elif k.endswith("gamma"):
            v = rng.uniform(0.7, 1.3, s)
        elif k.endswith("embeddings"):
            v = rng.normal(0, 0.5, s)
        elif len(s) == 2 and not k.endswith("gru1/bias"):
            v = rng.uniform(-1, 1, s) * np.sqrt(6 / (s[0] + s[1]))
        else:
            v = rng.normal(0, 0.2, s)
        if "local_att/dnn/" in k:
            v = v * att_scale
        w[k] = v.astype(np.float32)
    return w


# the weights' seed per case: one at which the reference meets the preconditions of
# test_model_cases_are_well_conditioned (default 17)
WEIGHT_SEEDS = {("toy", "bn-dice-paper"): 19, ("wide", "defaults"): 18, ("wide", "bn-dice-paper"): 19}
ATT_SCALE = {("wide", "bn-dice-paper"): 4.0}


def model_weights(data, cfg, seed=None):
    m, _, _ = make_model(data, cfg, "cpu")
    rng = np.random.default_rng(WEIGHT_SEEDS.get((data, cfg), 17) if seed is None else seed)
    w = rand_weights(m.keras_weights(), rng, ATT_SCALE.get((data, cfg), 1.0))
    aw = rand_weights(m.auxiliary_nn.keras_weights(), rng) if m.auxiliary_nn is not None else None
    return w, aw


STATS = ("moving_mean", "moving_variance")


def _dice_train(z, w, prefix, moved):
    mean, var = z.mean(0), z.var(0, unbiased=False)
    p = torch.sigmoid((z - mean) / torch.sqrt(var + 1e-9))
    for s, v in zip(STATS, (mean, var)):
        moved[f"{prefix}bn/{s}"] = 0.99 * w[f"{prefix}bn/{s}"] + 0.01 * v.detach()
    return w[prefix + "dice_alpha"] * (1 - p) * z + p * z


def dien_step_ref(m, w, aw, x, y, lr=LR, masks=None, dt=F64, relu_pre=None):
    """One fit step restated in torch: (BCE losses [B], auxiliary loss, the
    weights after the step, the auxiliary net's after the step)."""
    tw = {k: _t(v, dt).requires_grad_(not k.endswith(STATS)) for k, v in w.items()}
    ta = {k: _t(v, dt).requires_grad_() for k, v in (aw or {}).items()}
    moved = {}
    tab = lambda c: tw[f"{m._table_names[c.embedding_name]}/embeddings"]
    rows = lambda cs: torch.cat([tab(c)[torch.as_tensor(np.asarray(x[c.name]))] for c in cs], -1)
    keys, q = rows(m.history_cols), rows(m.query_cols)
    B, T, D = keys.shape
    L = np.asarray(x[m.length_name])
    ev = m.evolution
    act, norm = ev.attention.att_activation, ev.attention.weight_normalization
    H1 = gru_t(keys, tw["gru1/kernel"], tw["gru1/recurrent_kernel"], tw["gru1/bias"])
    Q = q[:, None].expand(B, T, D)
    e = torch.cat([Q, H1, Q - H1, Q * H1], -1).reshape(B * T, 4 * D)

    def activation(z, a, prefix, i):
        if a == "dice":
            return _dice_train(z, tw, f"{prefix}dice{i}/", moved)
        if a == "relu" and relu_pre is not None:
            relu_pre.append(z.detach().numpy().copy())
        return torch.relu(z) if a == "relu" else torch.sigmoid(z)

    for i in range(len(ev.attention.att_hidden_units)):
        e = activation(e @ tw[ATT + f"dnn/kernel{i}"] + tw[ATT + f"dnn/bias{i}"], act, ATT + "dnn/", i)
    s = mask_scores_t((e @ tw[ATT + "kernel"] + tw[ATT + "bias"]).reshape(B, T), L, norm)
    hist = augru_t(H1, s, tw["gru2/kernel"], tw["gru2/recurrent_kernel"], ev.augru_update)
    pooled = []
    for c in m.pooled_cols:
        emb = tab(c)[torch.as_tensor(np.asarray(x[c.name]))]
        Lc = _t(np.asarray(x[c.length_name], np.float32), dt).reshape(-1, 1)
        mask = (torch.arange(c.maxlen)[None] < Lc).to(dt)[:, :, None]
        v = (emb * mask).sum(1)
        pooled.append(v / (Lc + float(np.float32(1e-8))) if c.combiner == "mean" else v)
    dense = [_t(np.asarray(x[c.name], np.float32), dt).reshape(B, -1) for c in m.dense_cols]
    e = torch.cat([tab(c)[torch.as_tensor(np.asarray(x[c.name]))] for c in m.sparse_cols] + pooled + [hist] + dense, -1)
    for i in range(len(m.dnn.hidden_units)):
        e = e @ tw[f"dnn/kernel{i}"] + tw[f"dnn/bias{i}"]
        if m.dnn.use_bn:
            mean, var = e.mean(0), e.var(0, unbiased=False)
            for sname, v in zip(STATS, (mean, var)):
                moved[f"dnn/bn{i}/{sname}"] = 0.99 * tw[f"dnn/bn{i}/{sname}"] + 0.01 * v.detach()
            e = (e - mean) / torch.sqrt(var + 1e-3) * tw[f"dnn/bn{i}/gamma"] + tw[f"dnn/bn{i}/beta"]
        e = activation(e, m.dnn.activation, "dnn/", i)
        if masks is not None:
            e = e * _t(masks[i], dt)
    z = (e @ tw["dense/kernel"] + tw["prediction_layer/global_bias"]).reshape(B)
    t = _t(y, dt)
    bce = torch.nn.functional.softplus(z) - t * z          # -t log sig(z) - (1 - t) log(1 - sig(z))
    total, aux = bce.mean(), None
    if m.use_negsampling:
        neg = rows(m.neg_history_cols)
        net = lambda v: (torch.sigmoid(torch.sigmoid(v @ ta["kernel0"] + ta["bias0"]) @ ta["kernel1"] + ta["bias1"])
                         @ ta["kernel2"] + ta["bias2"])[:, :, 0]
        zc, zn = net(torch.cat([H1[:, :-1], keys[:, 1:]], -1)), net(torch.cat([H1[:, :-1], neg[:, 1:]], -1))
        amask = (torch.arange(T - 1)[None] < torch.as_tensor(L).reshape(-1, 1) - 1).to(dt)
        sp = torch.nn.functional.softplus
        aux = ((sp(-zc) + sp(zn)) * amask).mean()           # -log p_click - log(1 - p_noclick), p = sig(z)
        total = total + float(m.alpha) * aux
    for k, v in tw.items():
        if k.startswith("dnn/kernel") and m.dnn.l2_reg:
            total = total + float(m.dnn.l2_reg) * (v ** 2).sum()
        if k.endswith("embeddings") and m._l2_reg_embedding:
            total = total + float(m._l2_reg_embedding) * (v ** 2).sum()
    train = [k for k, v in tw.items() if v.requires_grad]
    grads = torch.autograd.grad(total, [tw[k] for k in train] + list(ta.values()), allow_unused=True)
    new = {k: v.detach().numpy() for k, v in tw.items()}
    new.update({k: v.numpy() for k, v in moved.items()})
    for k, g in zip(train, grads):
        if g is not None:
            new[k] = new[k] - lr * g.numpy()
    new_a = {k: v.detach().numpy() - lr * g.numpy() for (k, v), g in zip(ta.items(), grads[len(train):])}
    return bce.detach().numpy(), (None if aux is None else float(aux.detach())), new, (new_a or None)


def _cpu_masks(m, B, step):
    if not m.dnn.dropout_rate:
        return None
    from tests.helpers import dropout_masks
    return dropout_masks(123, 1000 * step, B, m.dnn.hidden_units, m.dnn.dropout_rate)[0]


def test_model_gradients_match_finite_differences():
    """The loss the step descends (the mean of the per-sample losses plus alpha
    times the auxiliary loss; l2 off) against central differences, at three
    random elements of every weight the step trains: with lr 1 the reference
    step moves a weight by exactly its gradient."""
    m, x, y = make_model("toy", "negsampling", "cpu")
    m._l2_reg_embedding = 0
    w, aw = model_weights("toy", "negsampling")
    w64 = {k: v.astype(np.float64) for k, v in w.items()}
    a64 = {k: v.astype(np.float64) for k, v in aw.items()}
    _, _, new, new_a = dien_step_ref(m, w64, a64, x, y, lr=1.0)

    def f(wv, av):
        bce, aux, _, _ = dien_step_ref(m, wv, av, x, y, lr=0.0)
        return float(bce.mean()) + m.alpha * aux

    rng = np.random.default_rng(2)
    for name in list(w64) + ["aux:" + k for k in a64]:
        src, key = (a64, name[4:]) if name.startswith("aux:") else (w64, name)
        if key.endswith(STATS):
            continue
        got = src[key] - (new_a if src is a64 else new)[key]       # lr 1: the gradient
        for _ in range(3):
            j = tuple(rng.integers(0, s) for s in src[key].shape)
            hi, lo = {k: v.copy() for k, v in src.items()}, {k: v.copy() for k, v in src.items()}
            hi[key][j] += 1e-6
            lo[key][j] -= 1e-6
            fd = (f(hi, a64) - f(lo, a64)) if src is w64 else (f(w64, hi) - f(w64, lo))
            assert abs(got[j] - fd / 2e-6) <= 1e-6 * max(1.0, abs(got[j])), (name, j)


def _check_conditioning(m, w, aw, batches):
    """The reference's steps over ``batches`` = [(x, y, masks)] in float32
    against float64: after every step the losses, the auxiliary loss and every
    weight within RTOL / 4; no relu pre-activation within 1e-4 of 0."""
    w32, a32 = w, aw
    for step, (x, y, masks) in enumerate(batches):
        pre = []
        bce, aux, w, aw = dien_step_ref(m, w, aw, x, y, masks=masks, relu_pre=pre)
        b32, x32, w32, a32 = dien_step_ref(m, w32, a32, x, y, masks=masks, dt=torch.float32)
        assert all(np.min(np.abs(p)) > 1e-4 for p in pre), f"step {step}: a relu pre-activation next to 0"
        for k in w:
            e = scaled_err(w32[k], w[k])
            assert e <= RTOL / 4, f"step {step} {k}: {e:.2e}"
        for k in (aw or {}):
            assert scaled_err(a32[k], aw[k]) <= RTOL / 4, f"step {step} aux {k}"
        assert scaled_err(b32, bce) <= RTOL / 4, f"step {step} losses"
        if aux is not None:
            assert abs(x32 - aux) <= RTOL / 4 * abs(aux), f"step {step} auxiliary loss"
        w32 = {k: np.asarray(v, np.float32) for k, v in w32.items()}
        a32 = a32 and {k: np.asarray(v, np.float32) for k, v in a32.items()}


@pytest.mark.parametrize("data,cfg", MODEL_CASES)
def test_model_cases_are_well_conditioned(data, cfg):
    """The three steps of test_train_steps_follow_the_reference."""
    m, x, y = make_model(data, cfg, "cpu")
    w, aw = model_weights(data, cfg)
    _check_conditioning(m, w, aw, [(x, y, _cpu_masks(m, len(y), step)) for step in range(STEPS)])


def compile_fit_batches():
    """test_compile_fit_takes_dien's data: the toy rows repeated to 96, batches
    of 32, 3 epochs — 9 sequential steps."""
    _, x, y = make_model("toy", "defaults", "cpu")
    X = {k: np.concatenate([v] * 32) for k, v in x.items()}
    Y = np.concatenate([y] * 32)
    one = [({k: v[r0:r0 + 32] for k, v in X.items()}, Y[r0:r0 + 32], None) for r0 in range(0, 96, 32)]
    return X, Y, one * 3


def test_the_other_gpu_steps_are_well_conditioned():
    """The dropout=False step of test_dropout_argument_and_bad_ids and the 9
    steps of test_compile_fit_takes_dien."""
    m, x, y = make_model("wide", "l2-dropout", "cpu")
    _check_conditioning(m, *model_weights("wide", "l2-dropout"), [(x, y, None)])
    m = make_model("toy", "defaults", "cpu")[0]
    _check_conditioning(m, *model_weights("toy", "defaults"), compile_fit_batches()[2])


def test_train_step_limits_on_the_cpu():
    cols, x, y = toy_data(False)
    m = rs.DIEN(cols, HIST, dnn_hidden_units=(4,), device="cpu")
    with pytest.raises(NotImplementedError, match="training runs only on a HIP device"):
        m.train_step(x, y)
    assert m.auxiliary_nn is None and m.last_aux_loss is None
    mn = rs.DIEN(toy_columns(True), HIST, use_negsampling=True, dnn_hidden_units=(4,), device="cpu")
    assert {k: tuple(v.shape) for k, v in mn.auxiliary_nn.keras_weights().items()} == {
        "kernel0": (24, 100), "bias0": (100,), "kernel1": (100, 50), "bias1": (50,), "kernel2": (50, 1), "bias2": (1,)}
    assert not any("auxiliary" in k for k in mn.keras_weights())
    # the same seed: every existing weight is the one the model without the net has
    a = rs.DIEN(toy_columns(True), HIST, use_negsampling=False, seed=5, device="cpu").keras_weights()
    b = rs.DIEN(toy_columns(True), HIST, use_negsampling=True, seed=5, device="cpu").keras_weights()
    assert sorted(a) == sorted(b) and all(torch.equal(a[k], b[k]) for k in a)


def _limit_model(**kw):
    cols = kw.pop("cols", None) or toy_columns(bool(kw.get("use_negsampling")))
    m = rs.DIEN(cols, HIST, dnn_hidden_units=(4,), device="cpu", **kw)
    m._dev = torch.device("cuda")   # the limits are checked before anything touches the device
    return m


def test_train_step_names_its_limits():
    _, x, y = toy_data(False)
    for kw, exc, word in [(dict(dnn_activation="sigmoid"), NotImplementedError, "dnn_activation"),
                          (dict(task="regression"), NotImplementedError, "binary")]:
        with pytest.raises(exc, match=word):
            _limit_model(**kw).train_step(x, y)
    S, V = rs.SparseFeat, rs.VarLenSparseFeat
    cols = toy_columns() + [V(S("tags", 7, embedding_dim=5), maxlen=6, combiner="max", length_name="tag_len")]
    with pytest.raises(NotImplementedError, match="max"):
        _limit_model(cols=cols).train_step(x, y)
    one = [S("item_id", 4, embedding_dim=8), S("cate_id", 3, embedding_dim=4)] + [
        V(S(p + "hist_" + n, v, embedding_dim=d, embedding_name=n), maxlen=1, length_name="seq_length")
        for p in ("", "neg_") for n, v, d in (("item_id", 4, 8), ("cate_id", 3, 4))]
    with pytest.raises(ValueError, match="T >= 2"):
        _limit_model(cols=one, use_negsampling=True).train_step(x, y)


# ------------------------------------------------------------------ GPU model
def _load(m, w, aw):
    m.set_keras_weights(w)
    if aw is not None:
        m.auxiliary_nn.set_keras_weights(aw)


def _compare(m, w, aw, what):
    for k, v in m.keras_weights().items():
        assert_scaled_close(v, w[k], what=f"{what} {k}")
    if aw is not None:
        for k, v in m.auxiliary_nn.keras_weights().items():
            assert_scaled_close(v, aw[k], what=f"{what} auxiliary_nn {k}")


@gpu_test
@pytest.mark.parametrize("data,cfg", MODEL_CASES)
def test_train_steps_follow_the_reference(gpu, data, cfg):
    from recommender_system_amd import _train_ops
    from tests.helpers import dropout_masks
    m, x, y = make_model(data, cfg, gpu)
    w, aw = model_weights(data, cfg)
    _load(m, w, aw)
    ref_m = make_model(data, cfg, "cpu")[0]
    B = len(y)
    for step in range(STEPS):
        masks = None
        if m.dnn.dropout_rate:
            rng = _train_ops._dropout_rng(m)
            masks = dropout_masks(rng.seed, rng.offset, B, m.dnn.hidden_units, m.dnn.dropout_rate)[0]
        bce, aux, w, aw = dien_step_ref(ref_m, w, aw, x, y, masks=masks)
        loss = m.train_step(x, y, lr=LR, return_loss=True)
        assert_scaled_close(loss, bce, what=f"step {step} losses")
        if aux is None:
            assert m.last_aux_loss is None
        else:
            assert abs(float(m.last_aux_loss) - aux) <= RTOL * abs(aux)
        _compare(m, w, aw, f"step {step}")
    # the inference forward (moving statistics) on the trained weights
    at = m.evolution.attention
    want = dien_ref(ref_m, {k: np.asarray(v, np.float32) for k, v in w.items()}, x, len(m.dnn.hidden_units),
                    m.dnn.activation, m.dnn.use_bn, at.att_activation, at.weight_normalization, m.evolution.augru_update)
    assert_scaled_close(m(x), want, what="forward after training")


@gpu_test
def test_dropout_argument_and_bad_ids(gpu):
    m, x, y = make_model("wide", "l2-dropout", gpu)
    w, aw = model_weights("wide", "l2-dropout")
    _load(m, w, aw)
    m.train_step(x, y, lr=LR, dropout=False)
    off = {k: v.clone() for k, v in m.keras_weights().items()}
    _load(m, w, aw)
    m.train_step(x, y, lr=LR)                        # dropout=None: the layer's own rate
    assert not torch.equal(off["dnn/kernel1"], m.keras_weights()["dnn/kernel1"])
    # dropout=False is the step of a model without dropout
    ref = dien_step_ref(make_model("wide", "l2-dropout", "cpu")[0], w, aw, x, y)[2]
    for k, v in off.items():
        assert_scaled_close(v, ref[k], what=f"dropout=False {k}")
    _load(m, w, aw)
    before = {k: v.clone() for k, v in m.keras_weights().items()}
    bad = dict(x, hist_item_id=np.where(np.arange(7)[None] == 2, 6, x["hist_item_id"]))
    with pytest.raises(IndexError):
        m.train_step(bad, y, lr=LR, check_ids=True)
    for k, v in m.keras_weights().items():
        assert torch.equal(v, before[k]), k


@gpu_test
def test_compile_fit_takes_dien(gpu):
    """The toy data repeated to 96 rows, batches of 32, 3 epochs: the history
    is the reference's sequential steps' mean losses."""
    m, x, y = make_model("toy", "defaults", gpu)
    w, aw = model_weights("toy", "defaults")
    _load(m, w, aw)
    X, Y, batches = compile_fit_batches()
    from recommender_system_amd.train import compile_fit
    hist = compile_fit(m, X, None, Y, batch_size=32, epochs=3, sgd=LR)
    ref_m = make_model("toy", "defaults", "cpu")[0]
    want, losses = [], []
    for xb, yb, _ in batches:
        bce, _, w, aw = dien_step_ref(ref_m, w, aw, xb, yb)
        losses.append(bce)
        if len(losses) == 3:
            want.append(float(np.concatenate(losses).mean()))
            losses = []
    assert np.all(np.isfinite(hist))
    np.testing.assert_allclose(hist, want, rtol=RTOL)
    _compare(m, w, aw, "after compile_fit")
