"""DIEN (model/dien.py:54-169): GRU, AttentionSequencePoolingLayer scores and
AUGRU on the one-launch kernel (dien.hip), the stand-alone rs_gru_fwd /
rs_augru_fwd, the host layers and the model.

The fp64 restatement (evolution_ref, dien_ref) lives here, on the oracle's
Dense / Dice / BatchNormalization, and is pinned by hand-computed cases.  CPU
tests cover the restatement, the conditioning of every GPU case (the same
restatement in float32 numpy must sit within RTOL / 4 of the float64 one, so a
failure on the GPU is the kernel's and not the inputs'), the support / size
queries, the argument checks and the host API; nothing is launched.  GPU tests
compare H1, scores and hist at the project's tolerance (tests.helpers.RTOL)
and check the ABI's bit-exactness contracts."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import recommender_system_amd as rs
from oracle import ctr_oracle as O
from recommender_system_amd import _lib
from tests.helpers import RTOL, assert_rel_close, assert_scaled_close

gpu_test = pytest.mark.gpu

ATT = "attention_sequence_pooling_layer/local_att/"
MASKED = float(-2 ** 32 + 1)


def hsig(x):
    return np.clip(0.2 * x + 0.5, 0, 1)


def act_ref(e, w, prefix, i, act, dt):
    if act == "dice":
        return O.dice(e, w[f"{prefix}dice{i}/dice_alpha"], w[f"{prefix}dice{i}/bn/moving_mean"],
                      w[f"{prefix}dice{i}/bn/moving_variance"], eps=1e-9, dt=dt)
    return O.activation(e, act)


def gru_ref(x, kernel, recurrent, bias, dt=np.float64):
    """Keras GRU(reset_after=True, use_bias=True), gate order z r h: [B, T, U]."""
    x, W, U, b = (np.asarray(v, dt) for v in (x, kernel, recurrent, bias))
    B, T, _ = x.shape
    u = U.shape[0]
    h = np.zeros((B, u), dt)
    out = np.zeros((B, T, u), dt)
    for t in range(T):
        xi = x[:, t] @ W + b[0]
        hr = h @ U + b[1]
        z = O.sigmoid(xi[:, :u] + hr[:, :u])
        r = O.sigmoid(xi[:, u:2 * u] + hr[:, u:2 * u])
        hh = np.tanh(xi[:, 2 * u:] + r * hr[:, 2 * u:])
        h = z * h + (1 - z) * hh
        out[:, t] = h
    return out


def augru_ref(x, scores, kernel, recurrent, update="reference", dt=np.float64):
    """AUGRU over AUGRUCell (layer/activation.py:113-142): the last state [B, U]."""
    x, s, W, U = (np.asarray(v, dt) for v in (x, scores, kernel, recurrent))
    B, T, _ = x.shape
    u = U.shape[0]
    h = np.zeros((B, u), dt)
    for t in range(T):
        xi = x[:, t] @ W
        z = hsig(xi[:, :u] + h @ U[:, :u]) * s[:, t:t + 1]
        r = hsig(xi[:, u:2 * u] + h @ U[:, u:2 * u])
        hh = np.tanh(xi[:, 2 * u:] + (r * h) @ U[:, 2 * u:])
        h = z * h + (1 - z) * hh if update == "reference" else (1 - z) * h + z * hh
    return h


def scores_ref(q, keys, lengths, w, n_layers, act, norm, dt=np.float64):
    """AttentionSequencePoolingLayer(return_score=True): [B, T]."""
    q, keys = np.asarray(q, dt), np.asarray(keys, dt)
    B, T, D = keys.shape
    Q = np.repeat(q[:, None], T, 1)
    e = np.concatenate([Q, keys, Q - keys, Q * keys], -1)
    for i in range(n_layers):
        e = act_ref(O.dense(e, w[ATT + f"dnn/kernel{i}"], w[ATT + f"dnn/bias{i}"], None, dt=dt), w, ATT + "dnn/", i, act,
                    dt)
    s = O.dense(e, w[ATT + "kernel"], w[ATT + "bias"], None, dt=dt)[:, :, 0]
    valid = np.arange(T)[None] < np.asarray(lengths).reshape(-1, 1)
    if not norm:
        return np.where(valid, s, dt(0))
    s = np.where(valid, s, dt(MASKED))
    p = np.exp(s - s.max(1, keepdims=True))
    return p / p.sum(1, keepdims=True)


def evolution_ref(keys, q, lengths, w, n_layers, act, norm, update="reference", dt=np.float64):
    """interest_evolution (model/dien.py:54-80): (H1 [B, T, D], scores [B, T], hist [B, D])."""
    h1 = gru_ref(keys, w["gru1/kernel"], w["gru1/recurrent_kernel"], w["gru1/bias"], dt)
    s = scores_ref(q, h1, lengths, w, n_layers, act, norm, dt)
    return h1, s, augru_ref(h1, s, w["gru2/kernel"], w["gru2/recurrent_kernel"], update, dt)


def scaled_err(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    rms = float(np.sqrt(np.mean(ref ** 2)))
    return float(np.max(np.abs(got - ref) / np.maximum(np.abs(ref), rms)))


def _ints(v):
    return (C.c_int * max(len(v), 1))(*v)


def rand_evolution_weights(rng, D, att, act, din=None):
    """Keras-named float32 weights of InterestEvolution: glorot-sized kernels,
    small non-zero biases, Dice statistics away from (0, 1, 0)."""
    g = lambda a, b: (rng.uniform(-1, 1, (a, b)) * np.sqrt(6 / (a + b))).astype(np.float32)
    n = lambda s, *shape: rng.normal(0, s, shape).astype(np.float32)
    w = {"gru1/kernel": g(din or D, 3 * D), "gru1/recurrent_kernel": g(D, 3 * D), "gru1/bias": n(0.1, 2, 3 * D),
         "gru2/kernel": g(D, 3 * D), "gru2/recurrent_kernel": g(D, 3 * D)}
    dims = [4 * D] + list(att)
    for i, (a, b) in enumerate(zip(dims[:-1], dims[1:])):
        w[ATT + f"dnn/kernel{i}"], w[ATT + f"dnn/bias{i}"] = g(a, b), n(0.1, b)
        if act == "dice":
            w[ATT + f"dnn/dice{i}/dice_alpha"] = n(0.3, b)
            w[ATT + f"dnn/dice{i}/bn/moving_mean"] = n(0.3, b)
            w[ATT + f"dnn/dice{i}/bn/moving_variance"] = rng.uniform(0.5, 1.5, b).astype(np.float32)
    w[ATT + "kernel"], w[ATT + "bias"] = g(dims[-1], 1), n(0.1, 1)
    return w


class Case:
    pass


@functools.lru_cache(maxsize=None)
def make_case(B, T, D, act="dice", norm=True, att=(64, 16), update="reference", seed=0):
    """Weights, inputs and the fp64 reference, computed once per configuration
    and shared (never modified).  Lengths cover 0, 1, T and > T when the batch
    has the rows for them."""
    rng = np.random.default_rng([seed, B, T, D, len(att)])
    c = Case()
    c.B, c.T, c.D, c.act, c.norm, c.att, c.update = B, T, D, act, norm, tuple(att), update
    c.w = rand_evolution_weights(rng, D, att, act)
    c.keys = rng.normal(0, 0.5, (B, T, D)).astype(np.float32)
    c.q = rng.normal(0, 0.5, (B, D)).astype(np.float32)
    c.len = rng.integers(1, T + 1, B).astype(np.int32)
    for i, v in enumerate([T, 1, 0, T + 3][:B]):
        c.len[i] = v
    c.h1, c.scores, c.hist = evolution_ref(c.keys, c.q, c.len, c.w, len(att), act, norm, update)
    return c


TMAX36 = 50  # the largest T of the one-launch form at D 36: 4 * (16 T 48 + 32 * 48 + 16 T) <= 160 KiB

# every evolution case a GPU test runs (test_gpu_cases_are_well_conditioned)
FUSED_CASES = [
    dict(B=33, T=7, D=12, act="dice", norm=True),
    dict(B=17, T=20, D=36, act="sigmoid", norm=True),
    dict(B=1, T=1, D=16, act="relu", norm=True),
    dict(B=17, T=7, D=16, act="relu", norm=False),
    dict(B=5, T=7, D=12, act="sigmoid", norm=False),
    dict(B=5, T=20, D=36, act="dice", norm=False),
    dict(B=17, T=TMAX36, D=36, act="dice", norm=True),
    dict(B=33, T=7, D=12, act="dice", norm=True, update="paper"),
]
UNFUSED_CASES = [
    dict(B=17, T=TMAX36 + 1, D=36, act="dice", norm=True),
    dict(B=5, T=7, D=12, act="sigmoid", norm=True, att=()),
    dict(B=5, T=7, D=12, act="relu", norm=True, att=(32, 16, 8)),
]
_id = lambda k: "-".join(f"{a}{v}" for a, v in k.items()).replace(" ", "")


# ------------------------------------------------------------------ CPU
def test_gru_step_by_hand():
    """D 2, one step from h = 0, both bias rows in play.  x = [1, 2],
    W = [[1, 0, 0, 1, 1, 0], [0, 1, 1, 0, 0, 1]] so x W = [1, 2 | 2, 1 | 1, 2];
    bias[0] = [0, -2, -2, 0, 0, 0] -> xi = [1, 0 | 0, 1 | 1, 2]; h = 0 so
    hr = bias[1] = [0, 0 | 0, 0 | 1, -2].  z = sig([1, 0]), r = sig([0, 1]),
    hh = tanh([1 + 0.5 * 1, 2 + sig(1) * -2]), h = (1 - z) hh."""
    W = np.array([[1, 0, 0, 1, 1, 0], [0, 1, 1, 0, 0, 1]], float)
    b = np.array([[0, -2, -2, 0, 0, 0], [0, 0, 0, 0, 1, -2]], float)
    U = np.arange(12, dtype=float).reshape(2, 6)  # multiplies h = 0
    sig = lambda v: 1 / (1 + np.exp(-v))
    want = (1 - sig(np.array([1.0, 0.0]))) * np.tanh([1 + 0.5, 2 - 2 * sig(1.0)])
    got = gru_ref([[[1.0, 2.0]]], W, U, b)
    np.testing.assert_allclose(got[0, 0], want, rtol=1e-15)
    # a second step sees h U: h1 U + bias[1] enters z, r and (inside r *) hh
    got2 = gru_ref([[[1.0, 2.0], [0.0, 0.0]]], W, U, b)[0, 1]
    h1 = want
    hr = h1 @ U + b[1]
    z, r = sig(b[0, :2] + hr[:2]), sig(b[0, 2:4] + hr[2:4])
    np.testing.assert_allclose(got2, z * h1 + (1 - z) * np.tanh(b[0, 4:] + r * hr[4:]), rtol=1e-15)


def test_augru_cell_by_hand():
    """U 1, two steps so the second sees h != 0.  W = [2, 20, 0.5], U = [1, 1, 1].
    Step 1 (x = 1, h = 0): z_pre 2 -> hsig 0.9; r_pre 20 -> hsig clips to 1;
    hh = tanh(0.5).  Score 0: z = 0, h = hh exactly.  Score 1: z = 0.9,
    h = 0.1 hh.  'paper' with score 1: h = 0.9 hh; with score 0: h stays 0."""
    W, U = np.array([[2.0, 20.0, 0.5]]), np.array([[1.0, 1.0, 1.0]])
    hh = np.tanh(0.5)
    x = [[[1.0]]]
    assert augru_ref(x, [[0.0]], W, U)[0, 0] == hh
    np.testing.assert_allclose(augru_ref(x, [[1.0]], W, U)[0, 0], 0.1 * hh, rtol=1e-15)
    np.testing.assert_allclose(augru_ref(x, [[1.0]], W, U, "paper")[0, 0], 0.9 * hh, rtol=1e-15)
    assert augru_ref(x, [[0.0]], W, U, "paper")[0, 0] == 0.0
    # clipping below: r_pre = -20 + h -> 0, so hh ignores h; x = -1, h = hh from step 1 (score 0)
    x2 = [[[1.0], [-1.0]]]
    z2 = 0.5 * hsig(-2 + hh)  # score 0.5
    want = z2 * hh + (1 - z2) * np.tanh(-0.5 + 0.0 * hh)
    np.testing.assert_allclose(augru_ref(x2, [[0.0, 0.5]], W, U)[0, 0], want, rtol=1e-15)
    assert hsig(-2.6) == 0.0 and hsig(2.6) == 1.0 and hsig(0.0) == 0.5


def test_score_masks_by_hand():
    rng = np.random.default_rng(3)
    D, T = 4, 5
    w = rand_evolution_weights(rng, D, (8, 4), "sigmoid")
    keys = rng.normal(0, 1, (3, T, D))
    q = rng.normal(0, 1, (3, D))
    s0 = scores_ref(q, keys, [0, 0, 0], w, 2, "sigmoid", True)
    assert np.array_equal(s0, np.full((3, T), 1.0 / T))          # nothing valid: a uniform softmax, exactly 1 / T
    assert np.array_equal(scores_ref(q, keys, [0, 0, 0], w, 2, "sigmoid", False), np.zeros((3, T)))
    for norm in (True, False):
        full = scores_ref(q, keys, [T, T, T], w, 2, "sigmoid", norm)
        assert np.array_equal(scores_ref(q, keys, [T + 1, T + 9, 10 ** 6], w, 2, "sigmoid", norm), full)
        part = scores_ref(q, keys, [2, 2, 2], w, 2, "sigmoid", norm)
        assert np.all(part[:, 2:] == 0) and np.all(part[:, :2] != 0)   # e^(-2^32) underflows to exactly 0
    np.testing.assert_allclose(scores_ref(q, keys, [2, 3, T], w, 2, "sigmoid", True).sum(1), 1.0, rtol=1e-14)


@pytest.mark.parametrize("k", FUSED_CASES + UNFUSED_CASES, ids=_id)
def test_gpu_cases_are_well_conditioned(k):
    """The restatement in float32 numpy against the float64 one: within
    RTOL / 4 for H1, scores and hist, so the GPU comparison at RTOL measures
    the kernel.  (Un-normalised scores are unbounded and 1 - a z can leave
    [0, 1]; a case that fails here needs another seed or shape, not a wider
    bound.)"""
    c = make_case(**k)
    got = evolution_ref(c.keys, c.q, c.len, c.w, len(c.att), c.act, c.norm, c.update, dt=np.float32)
    for name, g, r in zip(("H1", "scores", "hist"), got, (c.h1, c.scores, c.hist)):
        e = scaled_err(g, r)
        print(f"{_id(k)} {name}: float32 numpy scaled error {e:.2e}")
        assert e <= RTOL / 4, f"{name}: {e:.2e}"


def lds_bytes(T, D):
    """The header's formula."""
    dp = (D + 15) // 16 * 16
    return 4 * (16 * T * dp + 32 * dp + 16 * T)


def expected_prepared_size(D, att):
    up = lambda v: (v + 15) // 16 * 16
    dp, a1, a2 = up(D), up(att[0]), up(att[1])
    return 2 * (6 * dp * dp + 6 * dp) + 3 * a1 * dp + 4 * a1 + a2 * a1 + 5 * a2 + 4


def test_queries_follow_the_header():
    lib = _lib.lib()
    h = _ints([64, 16])
    for D in (1, 12, 16, 17, 36, 64):
        tmax = max(t for t in range(1, 700) if lds_bytes(t, D) <= 160 * 1024)
        assert lds_bytes(tmax + 1, D) > 160 * 1024
        for act in (1, 3, 4):
            assert lib.rs_dien_evolution_ok(tmax, D, 2, h, act) == 1, (D, tmax)
            assert lib.rs_dien_evolution_ok(tmax + 1, D, 2, h, act) == 0, (D, tmax)
        assert lib.rs_dien_prepared_size(D, 2, h) == expected_prepared_size(D, (64, 16))
    assert max(t for t in range(1, 700) if lds_bytes(t, 36) <= 160 * 1024) == TMAX36
    assert lib.rs_dien_evolution_ok(7, 36, 2, _ints([128, 128]), 4) == 1
    assert lib.rs_dien_prepared_size(36, 2, _ints([80, 40])) == expected_prepared_size(36, (80, 40))
    for what, args in [("D 65", (7, 65, 2, h, 1)), ("D 0", (7, 0, 2, h, 1)), ("T 0", (0, 12, 2, h, 1)),
                       ("depth 1", (7, 12, 1, h, 1)), ("depth 3", (7, 12, 3, _ints([8, 8, 8]), 1)),
                       ("depth 0", (7, 12, 0, None, 1)), ("width 129", (7, 12, 2, _ints([129, 16]), 1)),
                       ("width 0", (7, 12, 2, _ints([64, 0]), 1)), ("prelu", (7, 12, 2, h, 2)),
                       ("linear", (7, 12, 2, h, 0))]:
        assert lib.rs_dien_evolution_ok(*args) == 0, what
    assert lib.rs_dien_prepared_size(65, 2, h) == -1 and b"rs_dien_prepared_size" in lib.rs_last_error_string()
    assert lib.rs_dien_prepared_size(12, 3, _ints([8, 8, 8])) == -1
    up = lambda v: (v + 15) // 16 * 16
    for din, u in [(12, 12), (5, 36), (64, 1)]:
        assert lib.rs_gru_prepared_size(din, u) == 3 * up(u) * up(din) + 3 * up(u) * up(u) + 6 * up(u)
    assert lib.rs_gru_prepared_size(65, 8) == -1 and lib.rs_gru_prepared_size(8, 0) == -1


def test_argument_validation_returns_an_error_code():
    """Every refusal comes back as RS_ERR_ARG before any device work (the
    pointers are never dereferenced: 1 stands for 'not null')."""
    lib = _lib.lib()
    h, p = _ints([64, 16]), C.c_void_p(1)
    evo = lambda **k: lib.rs_dien_evolution_fwd(*[{**dict(
        keys=p, kb=7 * 12, kt=12, q=p, qs=12, len=p, lk=0, T=7, D=12, n=2, h=h, act=4, norm=1, upd=0, prep=p, H1=None,
        sc=None, hist=p, hs=12, B=3, st=None), **k}[a] for a in
        ("keys", "kb", "kt", "q", "qs", "len", "lk", "T", "D", "n", "h", "act", "norm", "upd", "prep", "H1", "sc",
         "hist", "hs", "B", "st")])
    assert evo(B=0) == 0 and evo(B=0, keys=None, hist=None) == 0      # empty batch: nothing launched
    for k in (dict(keys=None), dict(q=None), dict(len=None), dict(prep=None), dict(hist=None), dict(kt=11),
              dict(kb=6 * 12 + 11), dict(qs=11), dict(hs=11), dict(lk=2), dict(T=0), dict(D=65), dict(n=3),
              dict(act=2), dict(upd=2), dict(T=600), dict(B=-1)):
        assert evo(**k) == -1, k
        assert b"rs_dien_evolution_fwd" in lib.rs_last_error_string(), k
    ia, la, pa = (lambda v: (C.c_int * len(v))(*v)), (lambda v: (C.c_int64 * len(v))(*v)), \
        (lambda v: (C.c_void_p * len(v))(*v))
    ids = lambda **k: lib.rs_dien_evolution_ids_fwd(*[{**dict(
        nf=2, w=ia([8, 4]), kinds=ia([0, 1]), hi=pa([1, 1]), hst=la([7, 7]), ci=pa([1, 1]), cst=la([1, 1]),
        tab=pa([1, 1]), voc=la([4, 3]), len=p, lk=1, T=7, D=12, n=2, h=h, act=4, norm=1, upd=0, prep=p, H1=None,
        sc=None, hist=p, hs=12, B=3, err=None, st=None), **k}[a] for a in
        ("nf", "w", "kinds", "hi", "hst", "ci", "cst", "tab", "voc", "len", "lk", "T", "D", "n", "h", "act", "norm",
         "upd", "prep", "H1", "sc", "hist", "hs", "B", "err", "st")])
    assert ids(B=0) == 0
    for k in (dict(nf=0), dict(nf=5), dict(w=ia([8, 3])), dict(kinds=ia([0, 3])), dict(hst=la([6, 7])),
              dict(voc=la([4, 0])), dict(tab=pa([1, None])), dict(hi=pa([None, 1])), dict(w=None), dict(D=13),
              dict(len=None)):
        assert ids(**k) == -1, k
        assert b"rs_dien_evolution_ids_fwd" in lib.rs_last_error_string(), k
    assert lib.rs_gru_fwd(p, 7 * 5, 5, 7, 5, 9, p, None, None, 0, 3, None) == -1      # neither output
    assert lib.rs_gru_fwd(p, 7 * 5, 4, 7, 5, 9, p, p, None, 0, 3, None) == -1         # t stride < din
    assert lib.rs_gru_fwd(p, 7 * 5, 5, 7, 5, 65, p, p, None, 0, 3, None) == -1
    assert lib.rs_gru_fwd(None, 0, 0, 7, 5, 9, None, None, None, 0, 0, None) == 0     # empty batch
    assert lib.rs_augru_fwd(p, 7 * 5, 5, None, 7, 7, 5, 9, 0, p, p, 9, 3, None) == -1  # no scores
    assert lib.rs_augru_fwd(p, 7 * 5, 5, p, 6, 7, 5, 9, 0, p, p, 9, 3, None) == -1     # scores stride < T
    assert lib.rs_augru_fwd(p, 7 * 5, 5, p, 7, 7, 5, 9, 2, p, p, 9, 3, None) == -1     # unknown update
    assert lib.rs_gru_prepare(5, 9, None, p, None, p, None) == -1
    assert lib.rs_dien_prepare(12, p, p, p, p, p, 2, h, 4, pa([1, 1]), pa([1, 1]), None, None, None, p, p, p,
                               None) == -1                                             # dice without its statistics
    assert lib.rs_dien_prepare(12, p, p, None, p, p, 2, h, 1, pa([1, 1]), pa([1, 1]), None, None, None, p, p, p,
                               None) == -1


def toy_columns(neg=False):
    """model/dien.py:172-213."""
    S, V, D = rs.SparseFeat, rs.VarLenSparseFeat, rs.DenseFeat
    cols = [S("user", 3, embedding_dim=10), S("gender", 2, embedding_dim=4), S("item_id", 3 + 1, embedding_dim=8),
            S("cate_id", 2 + 1, embedding_dim=4), D("pay_score", 1),
            V(S("hist_item_id", vocabulary_size=3 + 1, embedding_dim=8, embedding_name="item_id"), maxlen=4,
              length_name="seq_length"),
            V(S("hist_cate_id", 2 + 1, embedding_dim=4, embedding_name="cate_id"), maxlen=4, length_name="seq_length")]
    if neg:
        cols += [V(S("neg_hist_item_id", vocabulary_size=3 + 1, embedding_dim=8, embedding_name="item_id"), maxlen=4,
                   length_name="seq_length"),
                 V(S("neg_hist_cate_id", 2 + 1, embedding_dim=4, embedding_name="cate_id"), maxlen=4,
                   length_name="seq_length")]
    return cols


def toy_inputs(neg=False):
    x = {"user": np.array([0, 1, 2]), "gender": np.array([0, 1, 0]), "item_id": np.array([1, 2, 3]),
         "cate_id": np.array([1, 2, 2]), "pay_score": np.array([0.1, 0.2, 0.3]),
         "hist_item_id": np.array([[1, 2, 3, 0], [1, 2, 3, 0], [1, 2, 0, 0]]),
         "hist_cate_id": np.array([[1, 2, 2, 0], [1, 2, 2, 0], [1, 2, 0, 0]]), "seq_length": np.array([3, 3, 2])}
    if neg:
        x["neg_hist_item_id"], x["neg_hist_cate_id"] = x["hist_item_id"].copy(), x["hist_cate_id"].copy()
    return x


def test_feature_columns():
    s = rs.SparseFeat("a", 10)
    assert s == ("a", 10, 4, False, None, "int32", None, "a", "default_group", True)
    assert s._fields == ("name", "vocabulary_size", "embedding_dim", "use_hash", "vocabulary_path", "dtype",
                         "embeddings_initializer", "embedding_name", "group_name", "trainable")
    assert rs.SparseFeat("a", 10000, embedding_dim="auto").embedding_dim == 60
    assert rs.SparseFeat("h", 5, embedding_name="a").embedding_name == "a" and hash(s) == hash("a")
    v = rs.VarLenSparseFeat(s, 7)
    assert v == (s, 7, "mean", None, None, True) and v.name == "a" and v.vocabulary_size == 10
    assert v.embedding_dim == 4 and v.embedding_name == "a" and v.dtype == "int32" and v.trainable is True
    assert rs.DenseFeat("d") == ("d", 1, "float32", None)
    with pytest.raises(NotImplementedError):
        rs.SparseFeat("a", 10, use_hash=True)
    with pytest.raises(NotImplementedError):
        rs.VarLenSparseFeat(s, 7, weight_name="w")
    with pytest.raises(NotImplementedError):
        rs.DenseFeat("d", transform_fn=lambda x: x)
    assert rs.get_feature_names(toy_columns(True)) == [
        "user", "gender", "item_id", "cate_id", "pay_score", "hist_item_id", "seq_length", "hist_cate_id",
        "neg_hist_item_id", "neg_hist_cate_id"]
    with pytest.raises(TypeError):
        rs.get_feature_names([("a", 3)])


def test_model_weights_and_tables():
    m = rs.DIEN(toy_columns(), ["item_id", "cate_id"], dnn_hidden_units=[4, 4, 4], device="cpu")
    w = m.keras_weights()
    shapes = {k: tuple(v.shape) for k, v in w.items()}
    want = {"sparse_emb_user/embeddings": (3, 10), "sparse_emb_gender/embeddings": (2, 4),
            "sparse_seq_emb_hist_item_id/embeddings": (4, 8), "sparse_seq_emb_hist_cate_id/embeddings": (3, 4),
            "gru1/kernel": (12, 36), "gru1/recurrent_kernel": (12, 36), "gru1/bias": (2, 36),
            "gru2/kernel": (12, 36), "gru2/recurrent_kernel": (12, 36),
            ATT + "kernel": (16, 1), ATT + "bias": (1,), ATT + "dnn/kernel0": (48, 64), ATT + "dnn/bias0": (64,),
            ATT + "dnn/kernel1": (64, 16), ATT + "dnn/bias1": (16,),
            "dnn/kernel0": (39, 4), "dnn/bias0": (4,), "dnn/kernel1": (4, 4), "dnn/bias1": (4,),
            "dnn/kernel2": (4, 4), "dnn/bias2": (4,), "dense/kernel": (4, 1), "prediction_layer/global_bias": (1,)}
    for i, n in ((0, 64), (1, 16)):
        for s in ("dice_alpha", "bn/moving_mean", "bn/moving_variance"):
            want[ATT + f"dnn/dice{i}/{s}"] = (n,)
    assert shapes == want
    # one table per embedding_name: candidate and history lookups share it
    assert m.tables["item_id"] is w["sparse_seq_emb_hist_item_id/embeddings"] and len(m.tables) == 4
    assert abs(float(w["sparse_emb_user/embeddings"].std()) - 1e-4) < 5e-5           # N(0, 1e-4)
    u = w["gru1/recurrent_kernel"].double()
    assert torch.allclose(u @ u.T, torch.eye(12, dtype=torch.float64), atol=1e-6)   # orthogonal
    assert float(w["gru1/bias"].abs().max()) == 0 and float(w["gru1/kernel"].abs().max()) <= (6 / 48) ** 0.5
    # the round trip, and a strict set refusing a missing / unknown name
    rng = np.random.default_rng(0)
    new = {k: rng.normal(0, 1, s).astype(np.float32) for k, s in shapes.items()}
    m.set_keras_weights(new)
    for k, v in m.keras_weights().items():
        np.testing.assert_array_equal(v.numpy(), new[k])
    with pytest.raises(KeyError):
        m.set_keras_weights({k: v for k, v in new.items() if k != "gru2/kernel"})
    with pytest.raises(KeyError):
        m.set_keras_weights({**new, "gru3/kernel": new["gru2/kernel"]})
    m.set_keras_weights({"dense/kernel": np.ones((4, 1), np.float32)}, strict=False)
    assert float(m.keras_weights()["dense/kernel"].sum()) == 4
    # with the neg_ columns the live Embedding of the name is the last column's
    mn = rs.DIEN(toy_columns(True), ["item_id", "cate_id"], use_negsampling=True, device="cpu")
    assert "sparse_seq_emb_neg_hist_item_id/embeddings" in mn.keras_weights() and len(mn.tables) == 4
    assert mn.input_width == m.input_width == 10 + 4 + 8 + 4 + 12 + 1


def test_gru_type_and_arguments():
    a = rs.DIEN(toy_columns(), ["item_id", "cate_id"], gru_type="GRU", seed=7, device="cpu").keras_weights()
    b = rs.DIEN(toy_columns(), ["item_id", "cate_id"], gru_type="AUGRU", seed=7, device="cpu").keras_weights()
    assert sorted(a) == sorted(b) and all(torch.equal(a[k], b[k]) for k in a)   # gru_type reaches nothing
    c = rs.DIEN(toy_columns(), ["item_id", "cate_id"], seed=8, device="cpu").keras_weights()
    assert not torch.equal(a["gru2/kernel"], c["gru2/kernel"])
    with pytest.raises(ValueError):
        rs.DIEN(toy_columns(), ["item_id", "cate_id"], augru_update="other", device="cpu")
    with pytest.raises(ValueError):
        rs.DIEN(toy_columns(), ["item_id", "brand"], device="cpu")
    m = rs.DIEN(toy_columns(), ["item_id", "cate_id"], device="cpu")
    assert m.evolution.fused_ok(4) and m.tower_fused_ok()
    assert not rs.DIEN(toy_columns(), ["item_id", "cate_id"], att_hidden_units=(8, 8, 8), device="cpu"
                       ).evolution.fused_ok(4)
    assert not rs.DIEN(toy_columns(), ["item_id", "cate_id"], use_bn=True, device="cpu").tower_fused_ok()
    assert not rs.DIEN(toy_columns(), ["item_id", "cate_id"], dnn_activation="dice", device="cpu").tower_fused_ok()
    g = rs.GRU(5, return_sequences=True, device="cpu", seed=0, input_dim=3)
    assert {k: tuple(v.shape) for k, v in g.keras_weights().items()} == {
        "kernel": (3, 15), "recurrent_kernel": (5, 15), "bias": (2, 15)}
    au = rs.AUGRU(5, device="cpu", seed=0, input_dim=3)
    assert {k: tuple(v.shape) for k, v in au.keras_weights().items()} == {"kernel": (3, 15), "recurrent_kernel": (5, 15)}
    with pytest.raises(NotImplementedError):
        rs.GRU(65, device="cpu", input_dim=3)


# ------------------------------------------------------------------ GPU
def _dev(a, gpu):
    return torch.as_tensor(np.ascontiguousarray(a)).to(gpu)


def evolution_module(c, gpu):
    m = rs.InterestEvolution(c.D, c.att, c.act, c.norm, augru_update=c.update, device=gpu, seed=0)
    m.set_keras_weights(c.w)
    return m


def check_evolution(got, c, what):
    hist, h1, sc = got
    assert_scaled_close(h1, c.h1, what=what + " H1")
    assert_scaled_close(sc, c.scores, what=what + " scores")
    assert_scaled_close(hist, c.hist, what=what + " hist")


@gpu_test
@pytest.mark.parametrize("k", FUSED_CASES, ids=_id)
def test_fused_evolution(gpu, k):
    """One launch against the fp64 restatement, and forward_unfused against
    both (the fused launch equals the composition within tolerance)."""
    c = make_case(**k)
    m = evolution_module(c, gpu)
    assert m.fused_ok(c.T)
    fused = m.forward_fused(_dev(c.keys, gpu), _dev(c.q, gpu), c.len, want_h1=True, want_scores=True)
    check_evolution(fused, c, "fused")
    unf = m.forward_unfused(_dev(c.keys, gpu), _dev(c.q, gpu), c.len, want_h1=True, want_scores=True)
    check_evolution(unf, c, "unfused")
    assert_scaled_close(fused[0], unf[0].cpu().numpy(), rtol=2 * RTOL, what="fused vs unfused hist")


@gpu_test
@pytest.mark.parametrize("k", UNFUSED_CASES, ids=_id)
def test_refused_shapes_run_unfused(gpu, k):
    """T past the LDS cap, attention depth 0 and 3: forward takes the composition."""
    c = make_case(**k)
    m = evolution_module(c, gpu)
    assert not m.fused_ok(c.T)
    check_evolution(m(_dev(c.keys, gpu), _dev(c.q, gpu), c.len, want_h1=True, want_scores=True), c, "unfused")


@gpu_test
def test_rnn_entries_with_another_input_width(gpu):
    """rs_gru_fwd / rs_augru_fwd with din != units: 5 -> 20 (sequence and
    last state) and 20 -> 36 with random scores, both blends."""
    rng = np.random.default_rng(11)
    B, T = 19, 9
    x = rng.normal(0, 0.5, (B, T, 5)).astype(np.float32)
    w1 = rand_evolution_weights(rng, 20, (), "relu", din=5)
    g = rs.GRU(20, return_sequences=True, device=gpu, seed=0, input_dim=5)
    g.set_keras_weights({k[5:]: v for k, v in w1.items() if k.startswith("gru1/")})
    ref = gru_ref(x, w1["gru1/kernel"], w1["gru1/recurrent_kernel"], w1["gru1/bias"])
    seq = g(_dev(x, gpu))
    assert_scaled_close(seq, ref, what="GRU sequence")
    g.return_sequences = False
    assert torch.equal(g(_dev(x, gpu)), seq[:, -1])
    w2 = rand_evolution_weights(rng, 36, (), "relu", din=20)
    s = rng.uniform(0, 1, (B, T)).astype(np.float32)
    for upd in ("reference", "paper"):
        au = rs.AUGRU(36, augru_update=upd, device=gpu, seed=0, input_dim=20)
        au.set_keras_weights({"kernel": w2["gru1/kernel"], "recurrent_kernel": w2["gru1/recurrent_kernel"]})
        got = au(seq, _dev(s, gpu))
        assert_scaled_close(got, augru_ref(ref, s, w2["gru1/kernel"], w2["gru1/recurrent_kernel"], upd),
                            what="AUGRU " + upd)


@gpu_test
def test_hist_bits_do_not_depend_on_outputs_or_batch_split(gpu):
    c = make_case(B=33, T=7, D=12, act="dice", norm=True)
    m = evolution_module(c, gpu)
    keys, q, L = _dev(c.keys, gpu), _dev(c.q, gpu), _dev(c.len, gpu)
    full, h1, sc = m.forward_fused(keys, q, L, want_h1=True, want_scores=True)
    assert torch.equal(m.forward_fused(keys, q, L), full)
    assert torch.equal(m.forward_fused(keys, q, L, want_h1=True)[0], full)
    a = m.forward_fused(keys[:17], q[:17], L[:17], want_h1=True, want_scores=True)
    b = m.forward_fused(keys[17:], q[17:], L[17:], want_h1=True, want_scores=True)
    for whole, x, y in zip((full, h1, sc), a, b):
        assert torch.equal(torch.cat([x, y]), whole)
    # hist written in place into a wider buffer (the model's tower input)
    buf = torch.full((33, 40), 7.0, device=gpu)
    m.forward_fused(keys, q, L.to(torch.int64), out=buf[:, 5:17])
    assert torch.equal(buf[:, 5:17], full) and float(buf[:, :5].min()) == 7.0 and float(buf[:, 17:].min()) == 7.0


def ids_case(gpu, B=33, T=7, seed=5):
    rng = np.random.default_rng(seed)
    vocabs, widths = (11, 5, 9), (8, 3, 1)
    tabs = [rng.normal(0, 0.5, (v, k)).astype(np.float32) for v, k in zip(vocabs, widths)]
    hist = [rng.integers(0, v, (B, T)) for v in vocabs]
    cand = [rng.integers(0, v, B) for v in vocabs]
    dts = (np.int32, np.int64, np.float32)
    hist_d = [_dev(h.astype(d), gpu) for h, d in zip(hist, dts)]
    cand_d = [_dev(x.astype(d), gpu) for x, d in zip(cand, dts)]
    return tabs, hist, cand, hist_d, cand_d


@gpu_test
def test_ids_form_matches_dense_form_bitwise(gpu):
    """Three behaviour features (int32, int64 and float ids; widths 8 + 3 + 1)."""
    c = make_case(B=33, T=7, D=12, act="dice", norm=True)
    m = evolution_module(c, gpu)
    tabs, hist, cand, hist_d, cand_d = ids_case(gpu)
    keys = np.concatenate([t[h] for t, h in zip(tabs, hist)], -1)
    q = np.concatenate([t[x] for t, x in zip(tabs, cand)], -1)
    dense = m.forward_fused(_dev(keys, gpu), _dev(q, gpu), c.len, want_h1=True, want_scores=True)
    got = m.forward_ids(hist_d, cand_d, [_dev(t, gpu) for t in tabs], c.len, want_h1=True, want_scores=True)
    for a, b in zip(got, dense):
        assert torch.equal(a, b)
    ref = evolution_ref(keys, q, c.len, c.w, 2, c.act, c.norm)
    assert_scaled_close(got[0], ref[2], what="ids hist")


@gpu_test
def test_out_of_range_history_id_is_a_flagged_zero_row(gpu):
    c = make_case(B=33, T=7, D=12, act="dice", norm=True)
    m = evolution_module(c, gpu)
    tabs, hist, cand, hist_d, cand_d = ids_case(gpu)
    hist_d[0][4, 2] = 11          # == vocab
    hist_d[1][20, 0] = -1
    td = [_dev(t, gpu) for t in tabs]
    with pytest.raises(IndexError):
        m.forward_ids(hist_d, cand_d, td, c.len)
    got = m.forward_ids(hist_d, cand_d, td, c.len, check_ids=False)
    keys = np.concatenate([t[h] for t, h in zip(tabs, hist)], -1)
    keys[4, 2, :8] = 0
    keys[20, 0, 8:11] = 0
    q = np.concatenate([t[x] for t, x in zip(tabs, cand)], -1)
    assert torch.equal(got, m.forward_fused(_dev(keys, gpu), _dev(q, gpu), c.len))


@gpu_test
def test_graph_capture_replays_the_same_bits(gpu):
    c = make_case(B=33, T=7, D=12, act="dice", norm=True)
    m = evolution_module(c, gpu)
    keys, q, L = _dev(c.keys, gpu), _dev(c.q, gpu), _dev(c.len, gpu)
    eager = m.forward_fused(keys, q, L).clone()
    out = torch.zeros(33, 12, device=gpu)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        m.forward_fused(keys, q, L, out=out)   # warm-up on the side stream (prepared image, LDS opt-in)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        m.forward_fused(keys, q, L, out=out)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    q.add_(0.25)                               # replay reads the inputs where they are
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, m.forward_fused(keys, q, L))


def rand_model_weights(m, rng):
    """Random Keras-named weights of a built DIEN: tables N(0, 0.5), glorot-sized
    kernels, small biases, statistics away from their defaults."""
    w = {}
    for k, p in m.keras_weights().items():
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
        w[k] = v.astype(np.float32)
    return w


def dien_ref(m, w, x, n_dnn, dnn_act, use_bn, att_act, norm, update="reference"):
    """DIEN.call from Keras-named weights: the tower input is [sparse rows |
    pooled other var-len columns (SequencePoolingLayer, layer/sequence.py:
    56-85) | hist | dense]."""
    tab = lambda c: w[f"{m._table_names[c.embedding_name]}/embeddings"].astype(np.float64)
    keys = np.concatenate([tab(c)[np.asarray(x[c.name])] for c in m.history_cols], -1)
    q = np.concatenate([tab(c)[np.asarray(x[c.name])] for c in m.query_cols], -1)
    hist = evolution_ref(keys, q, x["seq_length"], w, len(m.evolution.attention.att_hidden_units), att_act, norm,
                         update)[2]
    rows = [tab(c)[np.asarray(x[c.name])] for c in m.sparse_cols]
    dense = [np.asarray(x[c.name], np.float32).astype(np.float64).reshape(len(hist), -1) for c in m.dense_cols]
    pooled = []
    for c in m.pooled_cols:
        emb = tab(c)[np.asarray(x[c.name])]
        L = np.asarray(x[c.length_name], np.float64).reshape(-1, 1)
        mask = (np.arange(c.maxlen)[None] < L)[:, :, None].astype(np.float64)
        if c.combiner == "max":
            pooled.append((emb - (1 - mask) * 1e9).max(1))
        else:
            v = (emb * mask).sum(1)
            pooled.append(v / (np.float32(L).astype(np.float64) + np.float64(np.float32(1e-8)))
                          if c.combiner == "mean" else v)
    e = np.concatenate(rows + pooled + [hist] + dense, -1)
    for i in range(n_dnn):
        e = O.dense(e, w[f"dnn/kernel{i}"], w[f"dnn/bias{i}"], None)
        if use_bn:
            e = O.batchnorm_inference(e, w[f"dnn/bn{i}/moving_mean"], w[f"dnn/bn{i}/moving_variance"],
                                      w[f"dnn/bn{i}/gamma"], w[f"dnn/bn{i}/beta"], eps=1e-3)
        e = act_ref(e, w, "dnn/", i, dnn_act, np.float64)
    return O.sigmoid(e @ w["dense/kernel"].astype(np.float64) + w["prediction_layer/global_bias"].astype(np.float64))


@gpu_test
@pytest.mark.parametrize("neg", [False, True])
def test_model_toy(gpu, neg):
    """The reference's own example (model/dien.py:172-229): T 4, D 8 + 4,
    lengths [3, 3, 2], with and without the neg_ columns (which change nothing
    in the forward)."""
    m = rs.DIEN(toy_columns(neg), ["item_id", "cate_id"], dnn_hidden_units=[4, 4, 4], gru_type="AUGRU",
                use_negsampling=neg, device=gpu, seed=1024)
    w = rand_model_weights(m, np.random.default_rng(21))
    m.set_keras_weights(w)
    x = toy_inputs(neg)
    ref = dien_ref(m, w, x, 3, "relu", False, "dice", True)
    y = m(x)
    assert tuple(y.shape) == (3, 1)
    assert_rel_close(y, ref, what="DIEN toy")
    assert_rel_close(m.forward_unfused(x), ref, what="DIEN toy, unfused")
    assert tuple(m({k: v[:0] for k, v in x.items()}).shape) == (0, 1)
    bad = dict(x, hist_item_id=np.array([[1, 2, 4, 0], [1, 2, 3, 0], [1, 2, 0, 0]]))
    with pytest.raises(IndexError):
        m(bad)


def wide_model(gpu, **kw):
    """T 20, D 24 + 12 = 36, B 17, lengths from 0 to past T."""
    S, V = rs.SparseFeat, rs.VarLenSparseFeat
    cols = [S("user", 50, embedding_dim=6), S("item", 40, embedding_dim=24), S("cate", 9, embedding_dim=12),
            rs.DenseFeat("price", 2),
            V(S("hist_item", 40, embedding_dim=24, embedding_name="item"), maxlen=20, length_name="seq_length"),
            V(S("hist_cate", 9, embedding_dim=12, embedding_name="cate"), maxlen=20, length_name="seq_length")]
    m = rs.DIEN(cols, ["item", "cate"], dnn_hidden_units=(32, 16), device=gpu, seed=3, **kw)
    rng = np.random.default_rng(33)
    B = 17
    x = {"user": rng.integers(0, 50, B), "item": rng.integers(0, 40, B), "cate": rng.integers(0, 9, B),
         "price": rng.normal(0, 1, (B, 2)).astype(np.float32), "hist_item": rng.integers(0, 40, (B, 20)),
         "hist_cate": rng.integers(0, 9, (B, 20)), "seq_length": rng.integers(1, 21, B)}
    x["seq_length"][:4] = [20, 1, 0, 25]
    w = rand_model_weights(m, rng)
    m.set_keras_weights(w)
    return m, w, x


@gpu_test
def test_model_with_batchnorm_tower(gpu):
    m, w, x = wide_model(gpu, use_bn=True, att_activation="sigmoid", att_hidden_units=(64, 16))
    assert m.evolution.fused_ok(20) and not m.tower_fused_ok()
    ref = dien_ref(m, w, x, 2, "relu", True, "sigmoid", True)
    assert_rel_close(m(x), ref, what="DIEN use_bn")
    assert_rel_close(m.forward_unfused(x), ref, what="DIEN use_bn, unfused")


@gpu_test
def test_model_with_dice_tower_and_paper_update(gpu):
    m, w, x = wide_model(gpu, dnn_activation="dice", augru_update="paper")
    assert not m.tower_fused_ok()
    ref = dien_ref(m, w, x, 2, "dice", False, "dice", True, update="paper")
    assert_rel_close(m(x), ref, what="DIEN dice tower")


@gpu_test
def test_model_pools_other_varlen_columns(gpu):
    """Three more var-len columns ('mean', 'sum', 'max'; their own length
    inputs, one of them sharing a SparseFeat's table) land between the sparse
    rows and hist; lengths 0 ('mean' / 'sum': a zero vector), 1 and maxlen
    included.  ('max' keeps lengths >= 1: an empty sequence pools to -1e9,
    layer/sequence.py:76-78, which only saturates the tower.)"""
    S, V = rs.SparseFeat, rs.VarLenSparseFeat
    cols = toy_columns() + [V(S("tags", 7, embedding_dim=5), maxlen=6, combiner="mean", length_name="tag_len"),
                            V(S("shops", 9, embedding_dim=3), maxlen=6, combiner="sum", length_name="tag_len"),
                            V(S("seen_users", 3, embedding_dim=10, embedding_name="user"), maxlen=6, combiner="max",
                              length_name="seen_len")]
    m = rs.DIEN(cols, ["item_id", "cate_id"], dnn_hidden_units=[8, 4], dnn_activation="sigmoid", device=gpu, seed=5)
    assert rs.get_feature_names(cols)[-5:] == ["tags", "tag_len", "shops", "seen_users", "seen_len"]
    assert m.input_width == 39 + 5 + 3 + 10 and m.tables["user"].shape == (3, 10) and m.tower_fused_ok()
    rng = np.random.default_rng(8)
    w = rand_model_weights(m, rng)
    m.set_keras_weights(w)
    x = dict(toy_inputs(), tags=rng.integers(0, 7, (3, 6)), shops=rng.integers(0, 9, (3, 6)),
             seen_users=rng.integers(0, 3, (3, 6)), tag_len=np.array([6, 1, 0]), seen_len=np.array([1, 6, 3]))
    ref = dien_ref(m, w, x, 2, "sigmoid", False, "dice", True)
    assert_rel_close(m(x), ref, what="DIEN with pooled columns")
    with pytest.raises(IndexError):
        m(dict(x, shops=np.full((3, 6), 9)))
    with pytest.raises(ValueError):
        rs.DIEN(toy_columns() + [V(S("tags", 7), maxlen=6)], ["item_id", "cate_id"], device=gpu)
