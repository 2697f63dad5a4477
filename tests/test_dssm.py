"""DSSM (model/dssm.py:17-90): var-len pooling from ids (rs_seq_pool_fwd), a
whole tower in one launch (rs_dssm_tower_fwd), rs_l2_normalize_fwd, the
in-batch softmax loss (rs_inbatch_softmax_fwd), the 'logistic' score, the host
layers and the model.

The fp64 restatement (pool_ref, l2_ref, tower_ref, inbatch_ref, dssm_ref) lives
here, on the oracle's Dense / activation / BatchNormalization, and is pinned by
hand-computed cases.  CPU tests cover the restatement, the conditioning of
every GPU case (the same restatement in float32 numpy must sit within RTOL / 4
of the float64 one, so a failure on the GPU is the kernel's and not the
inputs'), the support queries, the argument checks and the host API; nothing is
launched.  GPU tests compare pooled rows, embeddings and losses at the
project's tolerance (tests.helpers.RTOL) and check the ABI's bit-exactness
contracts."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import recommender_system_amd as rs
from oracle import ctr_oracle as O
from recommender_system_amd import _lib, layers
from tests.helpers import RTOL, assert_scaled_close

gpu_test = pytest.mark.gpu
S, V, D = rs.SparseFeat, rs.VarLenSparseFeat, rs.DenseFeat


# ------------------------------------------------------------ restatement
def rows_ref(table, ids, dt=np.float64):
    """Embedding rows; an id outside [0, vocab) is the kernels' zero row."""
    table, ids = np.asarray(table, dt), np.asarray(ids).astype(np.int64)
    ok = (ids >= 0) & (ids < table.shape[0])
    return table[np.where(ok, ids, 0)] * ok[..., None].astype(dt)


def pool_ref(e, mode, lengths=None, mask=None, dt=np.float64):
    """SequencePoolingLayer.call (layer/sequence.py:56-86) on e [B, T, E]: with
    lengths (supports_masking=False) or a mask [B, T] (supports_masking=True,
    the length is the mask's row sum).  Returns [B, E]."""
    e = np.asarray(e, dt)
    B, T, _ = e.shape
    if lengths is not None:
        L = np.asarray(lengths).reshape(B, 1)
        mask = np.arange(T)[None] < L
    else:
        mask = np.asarray(mask).reshape(B, T) != 0
        L = mask.sum(1, keepdims=True)
    m = mask.astype(dt)[:, :, None]
    if mode == "max":
        return (e - (1 - m) * dt(1e9)).max(1)
    s = (e * m).sum(1)
    if mode == "mean":
        s = s / (np.float32(L).astype(dt) + dt(np.float32(1e-8)))
    return s


def l2_ref(x, dt=np.float64):
    """tf.math.l2_normalize(x, axis=-1): x * rsqrt(max(sum x^2, 1e-12))."""
    x = np.asarray(x, dt)
    return x / np.sqrt(np.maximum((x * x).sum(-1, keepdims=True), dt(1e-12)))


def logq_of(item_count):
    """log Q as the reference builds it (layer/utils.py:208-209): float32 of a
    float64 division, then a float32 log."""
    return np.log((np.asarray(item_count) / np.sum(item_count)).astype(np.float32))


def inbatch_ref(u, v, idx, item_count, temperature, dt=np.float64):
    """InBatchSoftmaxLayer.call: the per-sample loss [B]."""
    u, v = np.asarray(u, dt), np.asarray(v, dt)
    z = (u / dt(temperature)) @ v.T - logq_of(item_count).astype(dt)[np.asarray(idx).reshape(-1)][None]
    mx = z.max(1, keepdims=True)
    return (mx[:, 0] + np.log(np.exp(z - mx).sum(1))) - np.diagonal(z)


def score_ref(u, v, temperature, dt=np.float64):
    return O.sigmoid((np.asarray(u, dt) * np.asarray(v, dt)).sum(-1) / dt(temperature))


def tower_ref(m, tw, prefix, w, x, dt=np.float64):
    """One tower from Keras-named weights: [sparse rows | pooled var-len | dense]
    -> DNN (Dense, BatchNormalization with use_bn, activation; last layer
    linear) -> l2_normalize."""
    tab = lambda c: w[f"{m._table_names[c.embedding_name]}/embeddings"]
    parts = [rows_ref(tab(c), x[c.name], dt) for c in tw.sparse_cols]
    for c in tw.varlen_cols:
        e = rows_ref(tab(c), x[c.name], dt)
        parts.append(pool_ref(e, c.combiner, x[c.length_name], dt=dt) if c.length_name is not None
                     else pool_ref(e, c.combiner, mask=np.asarray(x[c.name]) != 0, dt=dt))
    B = len(parts[0]) if parts else len(np.asarray(x[tw.dense_cols[0].name]))
    parts += [np.asarray(x[c.name], np.float32).astype(dt).reshape(B, -1) for c in tw.dense_cols]
    e = np.concatenate(parts, -1)
    n = len(tw.dnn.layers)
    for i, l in enumerate(tw.dnn.layers):
        e = O.dense(e, w[f"{prefix}/kernel{i}"], w[f"{prefix}/bias{i}"], None, dt=dt)
        if tw.dnn.use_bn:
            e = O.batchnorm_inference(e, w[f"{prefix}/bn{i}/moving_mean"], w[f"{prefix}/bn{i}/moving_variance"],
                                      w[f"{prefix}/bn{i}/gamma"], w[f"{prefix}/bn{i}/beta"], eps=1e-3, dt=dt)
        e = O.activation(e, l.activation if i < n - 1 else None)
    return l2_ref(e, dt)


def dssm_ref(m, w, x, dt=np.float64):
    """(user embedding, item embedding, model output [B, 1])."""
    u = tower_ref(m, m.user_tower, "dnn", w, x, dt)
    v = tower_ref(m, m.item_tower, "dnn_1", w, x, dt)
    if m.loss_type == "softmax":
        y = inbatch_ref(u, v, x[m.sampler_config.item_name], m.sampler_config.item_count, m.temperature, dt)
    else:
        y = score_ref(u, v, m.temperature, dt)
    return u, v, y[:, None]


def scaled_err(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    rms = float(np.sqrt(np.mean(ref ** 2)))
    return float(np.max(np.abs(got - ref) / np.maximum(np.maximum(np.abs(ref), rms), 1e-30)))  # (an all-zero case: 0)


def _ints(v):
    return (C.c_int * max(len(v), 1))(*v)


def _dev(a, gpu):
    return torch.as_tensor(np.ascontiguousarray(a)).to(gpu)


# ------------------------------------------------------------------ cases
POOL_B, POOL_T, POOL_E = (1, 17, 33), (1, 7, 50), (4, 20, 32)
MODES = ("sum", "mean", "max")


@functools.lru_cache(maxsize=None)
def pool_case(B, T, E, seed=0):
    """ids [B, T] over a vocab of 23 (zeros in the middle of rows), a table
    N(0, 0.5) (|x| < 32: 'max' is exact) and lengths covering T + 3, 0, 1, T."""
    rng = np.random.default_rng(1000 * B + 10 * T + E + seed)
    table = rng.normal(0, 0.5, (23, E)).astype(np.float32)
    ids = rng.integers(1, 23, (B, T))
    ids[rng.random((B, T)) < 0.3] = 0
    if T > 2:
        ids[:, 1] = 0
        ids[:, T - 1] = 5
    L = np.concatenate([[T + 3, 0, 1, T], rng.integers(0, T + 1, B)])[:B]
    return table, ids, L


IB_B, IB_E, IB_TEMP = (1, 15, 16, 17, 48, 272, 1041), (8, 18, 32, 64), (0.05, 1.0)


@functools.lru_cache(maxsize=None)
def inbatch_case(B, E, seed=0):
    """Unit-norm user / item rows, item ids with duplicates in the batch, counts >= 1."""
    rng = np.random.default_rng(7 * B + E + 100003 * seed)
    n_items = 57
    u = l2_ref(rng.normal(0, 1, (B, E))).astype(np.float32)
    v = l2_ref(rng.normal(0, 1, (B, E))).astype(np.float32)
    idx = rng.integers(0, n_items, B)
    if B > 2:
        idx[2], v[2] = idx[0], v[0]  # a duplicated item
    counts = rng.integers(1, 200, n_items)
    return u, v, idx, counts


@functools.lru_cache(maxsize=None)
def inbatch_expected(B, E, temp):
    u, v, idx, counts = inbatch_case(B, E)
    return inbatch_ref(u, v, idx, counts, temp)


def demo_columns(vu=30, vm=40, vg=12, T=50):
    """The reference's demo (model/dssm.py:126-138) at small vocabularies."""
    user = [S("user_id", vu, 16), S("gender", 3, 16), S("age", 8, 16), S("occupation", 22, 16), S("zip", 35, 16),
            V(S("hist_movie_id", vm, 32, embedding_name="movie_id"), T, "mean", "hist_len"),
            V(S("hist_genres", vg, 32, embedding_name="genres"), T, "mean", "hist_len")]
    item = [S("movie_id", vm, 32), S("genres", vg, 32)]
    return user, item


def demo_inputs(rng, B, vu=30, vm=40, vg=12, T=50):
    L = rng.integers(1, T + 1, B)
    L[:4] = [T, 1, 0, T + 3][:min(B, 4)]
    hist = rng.integers(1, vm, (B, T)) * (np.arange(T)[None] < L[:, None])
    histg = rng.integers(1, vg, (B, T)) * (np.arange(T)[None] < L[:, None])
    return {"user_id": rng.integers(1, vu, B), "gender": rng.integers(1, 3, B), "age": rng.integers(1, 8, B),
            "occupation": rng.integers(1, 22, B), "zip": rng.integers(1, 35, B), "hist_movie_id": hist,
            "hist_genres": histg, "hist_len": L, "movie_id": rng.integers(1, vm, B), "genres": rng.integers(1, vg, B)}


def odd_columns():
    """A DenseFeat piece, a 'sum' column pooled by its id mask (no length
    input), a 'max' column, an item tower without layers."""
    user = [S("user_id", 30, 6), D("price", 3),
            V(S("tags", 9, 20), 7, "sum"), V(S("seen", 11, 4), 5, "max", "seen_len")]
    item = [S("movie_id", 40, 10)]
    return user, item


def odd_inputs(rng, B):
    tags = rng.integers(1, 9, (B, 7))
    tags[rng.random((B, 7)) < 0.4] = 0
    return {"user_id": rng.integers(0, 30, B), "price": rng.normal(0, 1, (B, 3)).astype(np.float32), "tags": tags,
            "seen": rng.integers(0, 11, (B, 5)), "seen_len": rng.integers(1, 6, B), "movie_id": rng.integers(0, 40, B)}


def rand_weights(m, rng):
    """Random Keras-named weights: tables N(0, 0.5), glorot-sized kernels, small
    biases, statistics away from their defaults."""
    w = {}
    for k, p in m.keras_weights().items():
        s = tuple(p.shape)
        if k.endswith("moving_variance"):
            v = rng.uniform(0.5, 1.5, s)
        elif k.endswith("gamma"):
            v = rng.uniform(0.7, 1.3, s)
        elif k.endswith("embeddings"):
            v = rng.normal(0, 0.5, s)
        elif len(s) == 2:
            v = rng.uniform(-1, 1, s) * np.sqrt(6 / (s[0] + s[1]))
        else:
            v = rng.normal(0, 0.2, s)
        w[k] = v.astype(np.float32)
    return w


TOWER_B = (1, 16, 17, 37)
CASES = {
    # name: (columns, inputs, user hidden, item hidden, activation, use_bn, loss_type, seed)
    "demo": (demo_columns, demo_inputs, (128, 64, 32), (64, 32), "relu", False, "softmax", 1),
    "odd": (odd_columns, odd_inputs, (24, 10), (), "sigmoid", False, "logistic", 2),
    "bn": (demo_columns, demo_inputs, (64, 32), (64, 32), "relu", True, "softmax", 3),
}


@functools.lru_cache(maxsize=None)
def model_case(name, B=48):
    """(constructor arguments, weights, inputs, fp64 (u, v, y)) — built on the CPU."""
    cols, inputs, uh, ih, act, bn, loss, seed = CASES[name]
    rng = np.random.default_rng(seed)
    ucols, icols = cols()
    x = inputs(rng, B)
    sampler = rs.NegativeSampler("inbatch", 255, "movie_id", item_count=rng.integers(1, 50, 40).tolist())
    kw = dict(user_dnn_hidden_units=uh, item_dnn_hidden_units=ih, dnn_activation=act, dnn_use_bn=bn, loss_type=loss,
              sampler_config=sampler, seed=seed)
    m = rs.DSSM(ucols, icols, device="cpu", **kw)
    w = rand_weights(m, rng)
    return (ucols, icols, kw), w, x, dssm_ref(m, w, x), m


def gpu_model(name, gpu, B=48):
    (ucols, icols, kw), w, x, ref, _ = model_case(name, B)
    m = rs.DSSM(ucols, icols, device=gpu, **kw)
    m.set_keras_weights(w)
    return m, w, x, ref


def head(x, B):
    return {k: v[:B] for k, v in x.items()}


# -------------------------------------------------------------- CPU tests
def test_pool_ref_hand_computed():
    """2 x 3 x 2, lengths 0, 2 and > T, and the id-mask form."""
    e = np.array([[[1., 2.], [3., 4.], [5., 6.]], [[-1., 0.], [2., -2.], [4., 8.]]])
    np.testing.assert_allclose(pool_ref(e, "sum", [2, 0]), [[4, 6], [0, 0]], rtol=0, atol=0)
    np.testing.assert_allclose(pool_ref(e, "mean", [2, 0]), [[2, 3], [0, 0]], rtol=1e-8)
    np.testing.assert_allclose(pool_ref(e, "max", [2, 0]), [[3, 4], [4 - 1e9, 8 - 1e9]], rtol=0, atol=0)
    np.testing.assert_allclose(pool_ref(e, "sum", [5, 3]), [[9, 12], [5, 6]], rtol=0, atol=0)
    np.testing.assert_allclose(pool_ref(e, "mean", [5, 3]), [[1.8, 2.4], [5 / 3, 2]], rtol=1e-8)   # divides by 5
    np.testing.assert_allclose(pool_ref(e, "max", [5, 3]), [[5, 6], [4, 8]], rtol=0, atol=0)
    ids = np.array([[3, 0, 2], [0, 0, 0]])
    np.testing.assert_allclose(pool_ref(e, "sum", mask=ids != 0), [[6, 8], [0, 0]], rtol=0, atol=0)
    np.testing.assert_allclose(pool_ref(e, "mean", mask=ids != 0), [[3, 4], [0, 0]], rtol=1e-8)
    np.testing.assert_allclose(pool_ref(e, "max", mask=ids != 0), [[5, 6], [4 - 1e9, 8 - 1e9]], rtol=0, atol=0)
    # in float32 a masked row is exactly -1e9 (|x| < 32): what the kernel writes
    assert pool_ref(e, "max", [2, 0], dt=np.float32)[1].tolist() == [-1e9, -1e9]
    # an out-of-range id is a zero row
    np.testing.assert_array_equal(rows_ref(np.array([[1., 2.], [3., 4.]]), [1, 2, -1]), [[3, 4], [0, 0], [0, 0]])


def test_l2_ref_zero_row_and_unit_norm():
    y = l2_ref(np.array([[0., 0., 0.], [3., 0., 4.]]))
    np.testing.assert_allclose(y, [[0, 0, 0], [0.6, 0, 0.8]], rtol=1e-15, atol=0)
    assert l2_ref(np.array([[1e-7, 0.]]))[0, 0] == pytest.approx(1e-7 / 1e-6)  # below the 1e-12 floor: x * 1e6


def test_inbatch_ref_hand_computed():
    """B = 2, u = v = I, temperature 1, counts (1, 3): Q = (1/4, 3/4)."""
    eye = np.eye(2)
    got = inbatch_ref(eye, eye, [0, 1], [1, 3], 1.0)
    want = [np.log(4 * np.e + 4 / 3) - (1 + np.log(4)), np.log(4 + 4 * np.e / 3) - (1 + np.log(4 / 3))]
    np.testing.assert_allclose(got, want, rtol=1e-6)  # (log Q is a float32 log)
    # both samples on item 1: the duplicate is not masked
    got = inbatch_ref(eye, eye, [1, 1], [1, 3], 1.0)
    np.testing.assert_allclose(got, [np.log(np.e + 1) - 1] * 2, rtol=1e-6)
    assert logq_of([1, 3]).dtype == np.float32
    np.testing.assert_allclose(score_ref(eye, eye, 0.5), [1 / (1 + np.exp(-2))] * 2, rtol=1e-15)


def test_pooling_cases_are_well_conditioned():
    for B in POOL_B:
        for T in POOL_T:
            for E in POOL_E:
                table, ids, L = pool_case(B, T, E)
                for mode in MODES:
                    for kw in (dict(lengths=L), dict(mask=ids != 0)):
                        ref = pool_ref(rows_ref(table, ids), mode, **kw)
                        f32 = pool_ref(rows_ref(table, ids, np.float32), mode, dt=np.float32, **kw)
                        assert f32.dtype == np.float32
                        assert scaled_err(f32, ref) <= RTOL / 4, (B, T, E, mode)


def test_inbatch_cases_are_well_conditioned():
    worst = 0.0
    for B in IB_B:
        for E in IB_E:
            for temp in IB_TEMP:
                u, v, idx, counts = inbatch_case(B, E)
                f32 = inbatch_ref(u, v, idx, counts, temp, np.float32)
                assert f32.dtype == np.float32
                worst = max(worst, scaled_err(f32, inbatch_expected(B, E, temp)))
    assert worst <= RTOL / 4, worst


@pytest.mark.parametrize("name", sorted(CASES))
def test_model_cases_are_well_conditioned(name):
    _, w, x, ref, m = model_case(name)
    f32 = dssm_ref(m, w, x, np.float32)
    for a, b, what in zip(f32, ref, ("user", "item", "output")):
        assert a.dtype == np.float32
        assert scaled_err(a, b) <= RTOL / 4, (name, what, scaled_err(a, b))


def test_support_queries_at_their_caps():
    lib = _lib.lib()
    assert lib.rs_inbatch_softmax_ok(1) == 1 and lib.rs_inbatch_softmax_ok(512) == 1
    assert lib.rs_inbatch_softmax_ok(513) == 0 and lib.rs_inbatch_softmax_ok(0) == 0
    relu = [_lib.ACT["relu"], _lib.ACT["relu"], 0]
    ok = lambda n_p, dims, acts: lib.rs_dssm_tower_ok(n_p, len(dims) - 1, _ints(dims), _ints(acts))
    assert ok(7, [144, 128, 64, 32], relu) == 1
    assert ok(16, [144, 128, 64, 32], relu) == 1 and ok(17, [144, 128, 64, 32], relu) == 0
    assert ok(0, [144, 128, 64, 32], relu) == 0
    assert ok(1, [64], []) == 1 and ok(1, [1024], []) == 1 and ok(1, [1025], []) == 0   # no layer: the row alone
    assert ok(2, [1024, 1024, 32], relu[1:]) == 1 and ok(2, [1025, 64, 32], relu[1:]) == 0
    assert ok(2, [64, 1025, 32], relu[1:]) == 0
    assert ok(2, [64] + [16] * 8, [1] * 8) == 1 and ok(2, [64] + [16] * 9, [1] * 9) == 0
    assert ok(2, [64, 32, 16], [_lib.ACT["sigmoid"], 0]) == 1
    assert ok(2, [64, 32, 16], [_lib.ACT["prelu"], 0]) == 0            # prelu / dice / BN towers run unfused
    assert ok(2, [64, 32, 16], [4, 0]) == 0
    assert ok(2, [429, 256, 128, 64, 1], [1, 1, 1, 0]) == 0           # rs_mlp_fwd's split-K tail shape
    assert ok(2, [429, 256, 128, 64, 2], [1, 1, 1, 0]) == 1
    assert layers.seq_pool_ok(64) and layers.seq_pool_ok(61) and layers.seq_pool_ok(256)
    assert not layers.seq_pool_ok(66) and not layers.seq_pool_ok(260) and not layers.seq_pool_ok(0)


def _pool_args(E=8, T=5, kind=0, comb=1, src=1, stride=None, table=1, vocab=9, length=1, len_kind=0, mask=None,
               out=1, out_stride=None, col=0, n=1):
    p = lambda v: (C.c_void_p * 1)(v)
    return (n, _ints([E]), _ints([col]), _ints([T]), _ints([comb]), _ints([kind]), p(src),
            (C.c_int64 * 1)(T if stride is None else stride), p(table), (C.c_int64 * 1)(vocab), p(length),
            _ints([len_kind]), p(mask), C.c_void_p(out), E if out_stride is None else out_stride, 4, C.c_void_p(1),
            None)


def test_argument_validation_without_device():
    """Every new entry refuses bad arguments before any device work."""
    lib = _lib.lib()
    err = lambda: lib.rs_last_error_string()
    assert lib.rs_seq_pool_fwd(*_pool_args(n=0)) == -1 and b"1..8" in err()
    assert lib.rs_seq_pool_fwd(*_pool_args(n=9)) == -1
    assert lib.rs_seq_pool_fwd(*_pool_args(E=66)) == -1 and b"width" in err()
    assert lib.rs_seq_pool_fwd(*_pool_args(E=260)) == -1
    assert lib.rs_seq_pool_fwd(*_pool_args(T=0)) == -1
    assert lib.rs_seq_pool_fwd(*_pool_args(comb=3)) == -1 and b"combiner" in err()
    assert lib.rs_seq_pool_fwd(*_pool_args(kind=3)) == -1
    assert lib.rs_seq_pool_fwd(*_pool_args(src=None)) == -1
    assert lib.rs_seq_pool_fwd(*_pool_args(stride=4)) == -1 and b"stride" in err()
    assert lib.rs_seq_pool_fwd(*_pool_args(table=None)) == -1 and b"table" in err()
    assert lib.rs_seq_pool_fwd(*_pool_args(vocab=0)) == -1
    assert lib.rs_seq_pool_fwd(*_pool_args(len_kind=2)) == -1 and b"lengths" in err()
    assert lib.rs_seq_pool_fwd(*_pool_args(col=1)) == -1                       # past the output row
    assert lib.rs_seq_pool_fwd(*_pool_args(kind=-1, stride=40, length=None)) == -1 and b"mask" in err()
    assert lib.rs_seq_pool_fwd(*_pool_args(kind=-1, stride=39)) == -1          # dense rows need T * E
    assert lib.rs_seq_pool_fwd(*_pool_args(out=None)) == -1
    one = C.c_void_p(1)
    assert lib.rs_l2_normalize_fwd(one, 4, one, 4, 3, 0, None) == -1
    assert lib.rs_l2_normalize_fwd(one, 3, one, 4, 3, 4, None) == -1 and b"stride" in err()
    assert lib.rs_l2_normalize_fwd(None, 4, one, 4, 3, 4, None) == -1 and b"null" in err()
    assert lib.rs_l2_normalize_fwd(None, 4, None, 4, 0, 4, None) == 0          # nothing to launch
    ib = lambda **k: lib.rs_inbatch_softmax_fwd(*[{**dict(u=one, us=8, v=one, vs=8, idx=one, kind=0, logq=one, n=5,
                                                          temp=0.05, loss=one, B=4, E=8, err=one, st=None), **k}[a]
                                                  for a in ("u", "us", "v", "vs", "idx", "kind", "logq", "n", "temp",
                                                            "loss", "B", "E", "err", "st")])
    assert ib(E=513) == -1 and b"512" in err()
    assert ib(us=7) == -1 and ib(n=0) == -1 and ib(kind=2) == -1 and ib(temp=0.0) == -1 and ib(B=-1) == -1
    assert ib(u=None) == -1 and b"null" in err()
    assert ib(B=0, u=None, v=None, idx=None, logq=None, loss=None) == 0
    sc = lambda u=one, us=8, v=one, vs=8, temp=1.0, out=one, B=4, E=8: lib.rs_dssm_score_fwd(u, us, v, vs, temp, out,
                                                                                             B, E, None)
    assert sc(E=0) == -1 and sc(vs=7) == -1 and sc(temp=-1.0) == -1 and sc(out=None) == -1 and sc(B=0, u=None) == 0
    # the tower: one sparse piece of 8 columns + one sequence of 8 -> 16 -> (16, 4)
    p1 = lambda v: (C.c_void_p * 1)(v)

    def tower(n_pieces=1, widths=(8,), cols=(0,), seq_cols=(8,), dims=(16, 16, 4), acts=(1, 0), prepared=one, out=one,
              out_stride=4, batch=4, err_flag=one, table=one):
        return lib.rs_dssm_tower_fwd(
            n_pieces, _ints(widths), _ints(cols), _ints([0]), p1(1), (C.c_int64 * 1)(1), p1(table), (C.c_int64 * 1)(9),
            1, _ints([8]), _ints(seq_cols), _ints([5]), _ints([1]), _ints([0]), p1(1), (C.c_int64 * 1)(5), p1(1),
            (C.c_int64 * 1)(9), p1(1), _ints([0]), p1(None), len(dims) - 1, _ints(dims), _ints(acts), prepared, out,
            out_stride, batch, err_flag, None)

    assert tower(acts=(2, 0)) == -1 and b"rs_dssm_tower_ok" in err()
    assert tower(dims=(16, 2000, 4)) == -1
    assert tower(seq_cols=(4,)) == -1 and b"overlap" in err()
    assert tower(dims=(20, 16, 4)) == -1 and b"cover" in err()
    assert tower(table=None) == -1 and b"table" in err()
    assert tower(prepared=None) == -1 and tower(out=None) == -1 and tower(out_stride=3) == -1
    assert tower(err_flag=None) == -1
    assert tower(batch=-1) == -1
    assert tower(batch=0) == 0                                                 # validated, nothing launched


def test_constructor_errors_and_layer_api():
    with pytest.raises(ValueError, match="mode must be sum or mean"):
        rs.SequencePoolingLayer("avg", device="cpu")
    with pytest.raises(ValueError, match="must support masking"):
        rs.SequencePoolingLayer("sum", supports_masking=True, device="cpu")(torch.zeros(2, 3, 4))
    user, item = demo_columns()
    sampler = rs.NegativeSampler("inbatch", 255, "movie_id", item_count=[1] * 40)
    with pytest.raises(ValueError, match="`loss_type` must be `logistic` or `softmax`"):
        rs.DSSM(user, item, loss_type="hinge", sampler_config=sampler, device="cpu")
    with pytest.raises(ValueError, match="sampler_config"):
        rs.DSSM(user, item, device="cpu")
    with pytest.raises(ValueError, match="item_name"):
        rs.DSSM(user, item, sampler_config=rs.NegativeSampler("inbatch", 255, "user_id", item_count=[1]), device="cpu")
    with pytest.raises(ValueError, match="output widths"):
        rs.DSSM(user, item, (64, 32), (64, 16), sampler_config=sampler, device="cpu")
    with pytest.raises(ValueError, match="does not match the table"):
        rs.DSSM(user, [S("movie_id", 41, 32)], sampler_config=sampler, device="cpu")
    with pytest.raises(NotImplementedError):   # weighted sequences and hashed ids are refused where the column is made
        V(S("hist_movie_id", 40, 32), 50, "mean", "hist_len", weight_name="w")
    with pytest.raises(NotImplementedError):
        S("movie_id", 40, 32, use_hash=True)
    with pytest.raises(ValueError, match="mode must be sum or mean"):
        rs.DSSM([V(S("h", 40, 32), 5, "avg")], [S("movie_id", 40, 32)], loss_type="logistic", device="cpu")
    m = rs.DSSM(user, item, (128, 64, 32), (64, 32), sampler_config=sampler, device="cpu")
    assert m.user_tower.input_width == 5 * 16 + 2 * 32 and m.item_tower.input_width == 64
    assert m.user_tower.fused_ok() and m.item_tower.fused_ok()
    assert not rs.DSSM(user, item, dnn_use_bn=True, sampler_config=sampler, device="cpu").user_tower.fused_ok()
    assert not rs.DSSM(user, item, dnn_activation="dice", sampler_config=sampler, device="cpu").user_tower.fused_ok()
    assert not rs.DSSM(user, item, dnn_activation="prelu", sampler_config=sampler, device="cpu").user_tower.fused_ok()
    # log Q: float32(count / sum) in float64, then a float32 log
    lay = rs.InBatchSoftmaxLayer(sampler._replace(item_count=[1, 3, 6])._asdict(), 0.05, device="cpu")
    assert lay.logq.dtype == torch.float32
    np.testing.assert_array_equal(lay.logq.numpy(), np.log(np.array([0.1, 0.3, 0.6]).astype(np.float32)))
    with pytest.raises(_lib.RSError, match="device"):   # no CPU fallback
        m(demo_inputs(np.random.default_rng(0), 4))


def test_keras_weights_round_trip_and_shared_tables():
    user, item = demo_columns()
    sampler = rs.NegativeSampler("inbatch", 255, "movie_id", item_count=[1] * 40)
    m = rs.DSSM(user, item, (128, 64, 32), (64, 32), sampler_config=sampler, device="cpu")
    names = set(m.keras_weights())
    # movie_id / genres: one table each, named after the var-len column that replaced the entry
    assert {n for n in names if n.endswith("embeddings")} == {
        "sparse_emb_user_id/embeddings", "sparse_emb_gender/embeddings", "sparse_emb_age/embeddings",
        "sparse_emb_occupation/embeddings", "sparse_emb_zip/embeddings", "sparse_seq_emb_hist_movie_id/embeddings",
        "sparse_seq_emb_hist_genres/embeddings"}
    assert {f"dnn/kernel{i}" for i in range(3)} | {"dnn_1/kernel0", "dnn_1/kernel1", "dnn_1/bias1"} <= names
    assert "dnn/kernel3" not in names and "dnn_1/kernel2" not in names
    assert m.tables["movie_id"].shape == (40, 32) and len(m.tables) == 7
    w = rand_weights(m, np.random.default_rng(4))
    m.set_keras_weights(w)
    for k, p in m.keras_weights().items():
        np.testing.assert_array_equal(p.numpy(), w[k])
    with pytest.raises(KeyError):
        m.set_keras_weights({k: v for k, v in w.items() if k != "dnn_1/bias0"})
    bn = rs.DSSM(user, item, (64,), (), loss_type="logistic", dnn_use_bn=True, device="cpu")   # no item layer
    assert "dnn/bn0/gamma" in bn.keras_weights() and not any(k.startswith("dnn_1/") for k in bn.keras_weights())
    assert bn.item_tower.out_width == 64 and bn.item_tower.fused_ok() and not bn.user_tower.fused_ok()


def test_negative_sampler_validation():
    with pytest.raises(ValueError, match="`softmax` sampler is not supported"):
        rs.NegativeSampler("softmax", 5, "movie_id", item_count=[1])
    with pytest.raises(ValueError, match="`item_count` must not be `None`"):
        rs.NegativeSampler("inbatch", 5, "movie_id")
    with pytest.raises(ValueError, match="`item_count` must not be `None`"):
        rs.NegativeSampler("frequency", 5, "movie_id")
    s = rs.NegativeSampler("uniform", 5, "movie_id")
    assert s.item_count is None and s.distortion == 1.0 and s._asdict()["item_name"] == "movie_id"
    assert float(rs.sampledsoftmaxloss(None, torch.tensor([[1.0], [3.0]]))) == 2.0
    assert rs.recall_N([1, 2, 3, 4], [4, 9, 1, 7], N=2) == 0.25


# -------------------------------------------------------------- GPU tests
def _pool(gpu, feats, B, width):
    """rs_seq_pool_fwd over feats into a fresh [B, width] buffer filled with 7."""
    out = torch.full((B, width), 7.0, device=gpu)
    err = layers._ErrFlag(gpu)
    layers.seq_pool(feats, out, B, err)
    return out, int(err.t.item())


@gpu_test
@pytest.mark.parametrize("mode", MODES)
def test_seq_pool_from_ids(gpu, mode):
    """Every B x T x E: lengths (T + 3, 0, 1, T, ...) with int32 ids and int32
    lengths, the id-mask form with int64 ids, and a split of the batch."""
    for B in POOL_B:
        for T in POOL_T:
            for E in POOL_E:
                table, ids, L = pool_case(B, T, E)
                td, e = _dev(table, gpu), rows_ref(table, ids)
                i32, i64 = _dev(ids.astype(np.int32), gpu), _dev(ids.astype(np.int64), gpu)
                got, flag = _pool(gpu, [(E, 0, T, mode, i32, td, _dev(L.astype(np.int32), gpu), None)], B, E)
                assert flag == 0
                assert_scaled_close(got, pool_ref(e, mode, L), what=f"{mode} lengths {B}x{T}x{E}")
                got64, _ = _pool(gpu, [(E, 0, T, mode, i64, td, _dev(L.astype(np.int64), gpu), None)], B, E)
                assert torch.equal(got64, got)
                masked, flag = _pool(gpu, [(E, 0, T, mode, i64, td, None, None)], B, E)
                assert flag == 0
                assert_scaled_close(masked, pool_ref(e, mode, mask=ids != 0), what=f"{mode} id mask {B}x{T}x{E}")
                if B > 1:   # 1 + (B - 1)
                    a, _ = _pool(gpu, [(E, 0, T, mode, i64[:1], td, None, None)], 1, E)
                    b, _ = _pool(gpu, [(E, 0, T, mode, i64[1:], td, None, None)], B - 1, E)
                    assert torch.equal(torch.cat([a, b]), masked)


@gpu_test
def test_seq_pool_two_features_dense_source_and_float_ids(gpu):
    """Two features of different T and E (and id kinds) in one launch, written
    into their columns of a wider buffer; the dense-values source with lengths
    and with a mask."""
    B = 33
    t1, i1, L1 = pool_case(B, 50, 32)
    t2, i2, L2 = pool_case(B, 7, 20)
    f1 = (32, 3, 50, "mean", _dev(i1.astype(np.int32), gpu), _dev(t1, gpu), _dev(L1, gpu), None)
    f2 = (20, 40, 7, "max", _dev(i2.astype(np.float32), gpu), _dev(t2, gpu), None, None)
    out, flag = _pool(gpu, [f1, f2], B, 64)
    assert flag == 0
    assert_scaled_close(out[:, 3:35], pool_ref(rows_ref(t1, i1), "mean", L1), what="feature 0")
    assert_scaled_close(out[:, 40:60], pool_ref(rows_ref(t2, i2), "max", mask=i2 != 0), what="feature 1")
    assert float(out[:, :3].min()) == 7.0 and float(out[:, 35:40].max()) == 7.0 and float(out[:, 60:].min()) == 7.0
    one, _ = _pool(gpu, [f1], B, 64)
    assert torch.equal(one[:, 3:35], out[:, 3:35])           # a feature's result does not depend on its launch mates
    # the layer's own call: embedded values [B, T, E]
    e = rows_ref(t1, i1).astype(np.float32)
    for mode in MODES:
        lay = rs.SequencePoolingLayer(mode, device=gpu)
        y = lay([_dev(e, gpu), _dev(L1.reshape(-1, 1), gpu)])
        assert tuple(y.shape) == (B, 1, 32)
        assert_scaled_close(y[:, 0], pool_ref(e, mode, L1), what=f"dense {mode}")
        ids_form = lay.forward_ids(i1, _dev(t1, gpu), L1)
        assert torch.equal(ids_form, y[:, 0])                # the same rows, the same order
        masked = rs.SequencePoolingLayer(mode, supports_masking=True, device=gpu)
        ym = masked(_dev(e, gpu), mask=_dev(i1 != 0, gpu))
        assert_scaled_close(ym[:, 0], pool_ref(e, mode, mask=i1 != 0), what=f"dense mask {mode}")
        assert torch.equal(masked.forward_ids(i1, _dev(t1, gpu)), ym[:, 0])
    e5 = rows_ref(t2, i2).astype(np.float32)[:, :, :5]       # a width 4 does not divide
    y5 = rs.SequencePoolingLayer("sum", device=gpu)([_dev(e5, gpu), _dev(L2, gpu)])
    assert_scaled_close(y5[:, 0], pool_ref(e5, "sum", L2), what="dense E 5")
    assert tuple(rs.SequencePoolingLayer("sum", device=gpu)([_dev(e5[:0], gpu), _dev(L2[:0], gpu)]).shape) == (0, 1, 5)


@gpu_test
def test_seq_pool_out_of_range_id_is_a_flagged_zero_row(gpu):
    B, T, E = 17, 7, 20
    table, ids, L = pool_case(B, T, E)
    ids = ids.copy()
    L = np.full(B, T)
    ids[3, 2], ids[9, 0] = 23, -1            # == vocab, negative
    lay = rs.SequencePoolingLayer("sum", device=gpu)
    td = _dev(table, gpu)
    with pytest.raises(_lib.BadIdError):
        lay.forward_ids(ids, td, L)
    got = lay.forward_ids(ids, td, L, check_ids=False)
    assert_scaled_close(got, pool_ref(rows_ref(table, ids), "sum", L), what="zero rows")
    # a bad id at a masked position is never read
    L[3], L[9] = 2, 0
    out, flag = _pool(gpu, [(E, 0, T, "sum", _dev(ids, gpu), td, _dev(L, gpu), None)], B, E)
    assert flag == 0
    assert_scaled_close(out, pool_ref(rows_ref(table, ids), "sum", L), what="masked bad ids")


@gpu_test
@pytest.mark.parametrize("N", [1, 32, 100])
def test_l2_normalize_and_score(gpu, N):
    for B in (1, 17):
        rng = np.random.default_rng(N + B)
        x = rng.normal(0, 1, (B, N)).astype(np.float32)
        x[0] = 0                                             # a zero row stays zero
        y = layers.l2_normalize(_dev(x, gpu))
        assert_scaled_close(y, l2_ref(x), what=f"l2 {B}x{N}")
        assert float(y[0].abs().max()) == 0.0
        wide = torch.full((B, N + 3), 7.0, device=gpu)       # strided rows, in place
        wide[:, :N] = _dev(x, gpu)
        layers.l2_normalize(wide[:, :N], out=wide[:, :N])
        assert torch.equal(wide[:, :N], y) and float(wide[:, N:].min()) == 7.0
        u, v = l2_ref(rng.normal(0, 1, (B, N))).astype(np.float32), l2_ref(rng.normal(0, 1, (B, N))).astype(np.float32)
        ud, vd, out = _dev(u, gpu), _dev(v, gpu), torch.empty(B, 1, device=gpu)
        for temp in (0.05, 1.0):
            _lib.call("rs_dssm_score_fwd", _lib.ptr(ud), N, _lib.ptr(vd), N, temp, _lib.ptr(out), B, N, _lib.stream())
            assert_scaled_close(out[:, 0], score_ref(u, v, temp), what=f"score {B}x{N} t {temp}")


@gpu_test
@pytest.mark.parametrize("E", IB_E)
def test_inbatch_softmax(gpu, E):
    for B in IB_B:
        u, v, idx, counts = inbatch_case(B, E)
        sampler = rs.NegativeSampler("inbatch", 255, "movie_id", item_count=counts.tolist())
        ud, vd = _dev(u, gpu), _dev(v, gpu)
        for temp in IB_TEMP:
            lay = rs.InBatchSoftmaxLayer(sampler._asdict(), temp, device=gpu)
            got = lay([ud, vd, idx.reshape(-1, 1)])
            assert tuple(got.shape) == (B, 1)
            assert_scaled_close(got[:, 0], inbatch_expected(B, E, temp), what=f"loss B {B} E {E} t {temp}")
            assert torch.equal(lay([ud, vd, _dev(idx.astype(np.int32), gpu)]), got)     # run to run, int32 / int64
        if B > 2:
            assert idx[2] == idx[0]                          # the duplicated item is an ordinary column


@gpu_test
def test_inbatch_softmax_flags_an_item_index_out_of_range(gpu):
    B, E = 17, 18
    u, v, idx, counts = inbatch_case(B, E)
    lay = rs.InBatchSoftmaxLayer(rs.NegativeSampler("inbatch", 255, "movie_id", item_count=counts.tolist()), 0.05,
                                 device=gpu)
    bad = idx.copy()
    bad[5] = len(counts)
    with pytest.raises(_lib.BadIdError):
        lay([u, v, bad])
    got = lay([u, v, bad], check_ids=False)
    # log Q = 0 for that column: the reference's formula with Q = 1 there
    z = (u.astype(np.float64) / 0.05) @ v.astype(np.float64).T
    lq = logq_of(counts).astype(np.float64)[np.where(bad < len(counts), bad, 0)]
    lq[5] = 0
    z = z - lq[None]
    ref = np.log(np.exp(z - z.max(1, keepdims=True)).sum(1)) + z.max(1) - np.diagonal(z)
    assert_scaled_close(got[:, 0], ref, what="logq 0")
    # strided rows: the embeddings as columns of a wider buffer
    wide_u, wide_v = torch.zeros(B, E + 5, device=gpu), torch.zeros(B, E + 2, device=gpu)
    wide_u[:, 5:], wide_v[:, :E] = _dev(u, gpu), _dev(v, gpu)
    loss, flag = torch.empty(B, device=gpu), torch.zeros(1, dtype=torch.int32, device=gpu)
    idx_d = _dev(idx, gpu)
    _lib.call("rs_inbatch_softmax_fwd", _lib.ptr(wide_u[:, 5:]), E + 5, _lib.ptr(wide_v), E + 2, _lib.ptr(idx_d), 1,
              _lib.ptr(lay.logq), len(counts), 0.05, _lib.ptr(loss), B, E, _lib.ptr(flag), _lib.stream())
    assert torch.equal(loss, lay([u, v, idx])[:, 0]) and int(flag.item()) == 0


@gpu_test
@pytest.mark.parametrize("name", ["demo", "odd"])
def test_tower_matches_fp64_and_the_unfused_composition(gpu, name):
    """'demo': the reference's towers (5 x 16 + 2 sequences x 32 at T 50 ->
    128 -> 64 -> 32; 2 x 32 -> 64 -> 32).  'odd': a DenseFeat piece, an
    id-masked 'sum' column, a 'max' column, 'sigmoid', hidden (24, 10) (no
    multiple of 16), and an item tower with no layer."""
    m, w, x, (u_ref, v_ref, _) = gpu_model(name, gpu, B=37)
    assert m.user_tower.fused_ok() and m.item_tower.fused_ok()
    for B in TOWER_B:
        xb = head(x, B)
        u, v = m.user_embedding(xb), m.item_embedding(xb)
        assert_scaled_close(u, u_ref[:B], what=f"{name} user B {B}")
        assert_scaled_close(v, v_ref[:B], what=f"{name} item B {B}")
        assert torch.equal(u, m.user_embedding(xb, fused=False))
        assert torch.equal(v, m.item_embedding(xb, fused=False))
        if B == 37:   # any split of the batch
            rest = {k: a[1:] for k, a in x.items()}
            assert torch.equal(torch.cat([m.user_embedding(head(x, 1)), m.user_embedding(rest)]), u)
    assert tuple(m.user_embedding(head(x, 0)).shape) == (0, u_ref.shape[1])


@gpu_test
@pytest.mark.parametrize("name", ["demo", "odd", "bn"])
def test_model(gpu, name):
    m, w, x, (u_ref, v_ref, y_ref) = gpu_model(name, gpu)
    fused = name != "bn"
    assert m.user_tower.fused_ok() == fused and m.item_tower.fused_ok() == fused
    y = m(x)
    assert tuple(y.shape) == (48, 1)
    assert_scaled_close(y, y_ref, what=f"DSSM {name}")
    assert_scaled_close(m.forward_unfused(x), y_ref, what=f"DSSM {name}, unfused")
    if fused:
        assert torch.equal(m.forward_unfused(x), y)
    u, v = m.user_embedding(x), m.item_embedding(x)
    assert_scaled_close(u, u_ref, what="user embedding")
    assert_scaled_close(v, v_ref, what="item embedding")
    one = torch.ones(48, device=gpu)
    assert torch.allclose(u.norm(dim=1), one, rtol=0, atol=1e-6) and torch.allclose(v.norm(dim=1), one, rtol=0, atol=1e-6)
    with pytest.raises(IndexError):
        m(dict(x, movie_id=np.full(48, 40)))
    assert tuple(m(head(x, 0)).shape) == (0, 1)


@gpu_test
def test_graph_capture_replays_the_same_bits(gpu):
    m, w, x, _ = gpu_model("demo", gpu)
    xd = {k: _dev(v, gpu) for k, v in x.items()}
    eager = m(xd).clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        m(xd, check_ids=False)                 # warm-up on the side stream (prepared images, LDS opt-in)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = m(xd, check_ids=False)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    xd["hist_len"].fill_(3)                    # replay reads the inputs where they are
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, m(xd))
