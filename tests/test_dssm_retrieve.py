"""DSSM retrieval: rs_topn_inner_product (csrc/topn.hip), retrieval.py and
DSSM.predict_*_embedding / retrieve / recall.

The operation is exact top-N by inner product under the total order (score
descending, item position ascending).  ``topn_ref`` restates it in numpy and
is pinned by a hand-computed case.

Exact inputs: entries that are multiples of 1/8 with |x| <= 2 and E <= 64 (the
one E = 256 case: |x| <= 1), so that every product is a multiple of 1/64 and
every partial sum stays below 2^9 — the scores are exact in fp32 in any
summation order, and positions and scores must equal ``topn_ref`` BITWISE,
from the kernel and from the torch composition alike.

Float inputs (l2-normalised Gaussian rows): near-ties make exact positions
unobtainable in fp32, so ``check_float_rule`` asks, for every user and rank,
that the returned score and the fp64 score of the returned position lie within
assert_scaled_close's bound of the reference's score at that rank, that the
positions are distinct and in range, and that every item whose fp64 score
clears the reference's N-th by more than twice the bound is present.  The
float32 numpy restatement passes the same rule at RTOL / 4 (the conditioning
rule)."""
import functools

import numpy as np
import pytest
import torch

import recommender_system_amd as rs
from recommender_system_amd import _lib, retrieval
from tests.helpers import RTOL, assert_scaled_close
from tests.test_dssm import l2_ref, rand_weights, tower_ref

gpu_test = pytest.mark.gpu
S, V = rs.SparseFeat, rs.VarLenSparseFeat


# ------------------------------------------------------------------ restatement
def topn_ref(u, v, N, dt=np.float64):
    """(positions int32 [U, N], scores dt [U, N]): scores in dt, ordered by
    (-score, position), padded with (-1, -inf)."""
    u, v = np.asarray(u, dt), np.asarray(v, dt)
    s = u @ v.T
    idx = np.full((len(u), N), -1, np.int32)
    score = np.full((len(u), N), -np.inf, dt)
    n = min(N, len(v))
    pos = np.arange(len(v))
    for i in range(len(u)):
        order = np.lexsort((pos, -s[i]))[:n]  # by -score, then by position
        idx[i, :n], score[i, :n] = order, s[i, order]
    return idx, score


def check_float_rule(idx, score, u, v, N, rtol, what):
    idx, score = np.asarray(idx), np.asarray(score, np.float64)
    U, I = len(u), len(v)
    assert idx.shape == (U, N) and score.shape == (U, N) and I >= N
    ref_idx, ref = topn_ref(u, v, N)
    assert_scaled_close(score, ref, rtol, what=f"{what}: scores")
    bound = rtol * np.maximum(np.abs(ref), float(np.sqrt(np.mean(ref ** 2))))
    s64 = np.asarray(u, np.float64) @ np.asarray(v, np.float64).T
    assert idx.min() >= 0 and idx.max() < I, f"{what}: a position out of range"
    assert all(len(set(r)) == N for r in idx.tolist()), f"{what}: a position twice"
    got64 = np.take_along_axis(s64, idx.astype(np.int64), 1)
    off = np.abs(got64 - ref)
    assert (off <= bound).all(), f"{what}: a returned item's fp64 score is {float((off / bound).max()):.2f} bounds off its rank"
    present = np.zeros((U, I), bool)
    np.put_along_axis(present, idx.astype(np.int64), True, 1)
    must = s64 > (ref[:, -1] + 2 * bound[:, -1])[:, None]
    assert not (must & ~present).any(), f"{what}: {int((must & ~present).sum())} clear winners are missing"


def exact(rng, shape, top=16):
    """multiples of 1/8 in [-top / 8, top / 8]"""
    return (rng.integers(-top, top + 1, shape) / 8).astype(np.float32)


def same_bits(idx, score, ref_idx, ref_score, what):
    idx, score = np.asarray(idx), np.asarray(score)
    assert idx.dtype == np.int32 and score.dtype == np.float32
    assert np.array_equal(idx, ref_idx), f"{what}: positions differ at {np.argwhere(idx != ref_idx)[:4].tolist()}"
    assert np.array_equal(score.view(np.int32), np.asarray(ref_score, np.float32).view(np.int32)), f"{what}: scores differ"


def test_topn_ref_hand_computed():
    u = np.array([[1, 0], [0, 1], [1, 1]], np.float32)
    v = np.array([[1, 0], [0, 2], [1, 0], [-1, -1], [0.5, 0.5]], np.float32)
    # scores: user 0: 1, 0, 1, -1, .5   user 1: 0, 2, 0, -1, .5   user 2: 1, 2, 1, -2, 1
    idx, score = topn_ref(u, v, 3)
    assert idx.tolist() == [[0, 2, 4], [1, 4, 0], [1, 0, 2]]
    assert score.tolist() == [[1, 1, 0.5], [2, 0.5, 0], [2, 1, 1]]
    idx, score = topn_ref(u, v[:2], 3, np.float32)
    assert idx.tolist() == [[0, 1, -1], [1, 0, -1], [1, 0, -1]] and score.dtype == np.float32
    assert score[:, :2].tolist() == [[1, 0], [2, 0], [2, 1]] and np.isneginf(score[:, 2]).all()
    idx, score = topn_ref(u, v[:0], 2)
    assert (idx == -1).all() and np.isneginf(score).all()


# ------------------------------------------------------------------ cases
@functools.lru_cache(maxsize=None)
def float_case(U=300, I=3707, E=32, seed=0):
    rng = np.random.default_rng(seed)
    return (l2_ref(rng.normal(0, 1, (U, E))).astype(np.float32), l2_ref(rng.normal(0, 1, (I, E))).astype(np.float32))


def ties_case(E, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(-1, 2, (37, E)).astype(np.float32), rng.integers(-1, 2, (1000, E)).astype(np.float32)


def _equal_scores():
    return np.ones((5, 8), np.float32), np.ones((200, 8), np.float32)


def _traffic(descending):
    v = (np.arange(5000, dtype=np.float32) / 16)[:, None]
    return np.ones((1, 1), np.float32), np.ascontiguousarray(v[::-1]) if descending else v


def _rand(U, I, E, N, seed, top=16):
    rng = np.random.default_rng(seed)
    return exact(rng, (U, E), top), exact(rng, (I, E), top), N


EXACT = {
    # name: () -> (user, item, N)
    "ties E18 (scalar loads)": lambda: (*ties_case(18, 1), 50),
    "ties E32 (vector loads)": lambda: (*ties_case(32, 2), 50),
    "all scores equal": lambda: (*_equal_scores(), 50),
    "ascending: every item is inserted": lambda: (*_traffic(False), 50),
    "descending: nothing after the first N": lambda: (*_traffic(True), 50),
    "N 1": lambda: _rand(20, 333, 24, 1, 3),
    "N 128, I 300": lambda: _rand(9, 300, 16, 128, 4),
    "I 10 < N 50": lambda: _rand(6, 10, 12, 50, 5),
    "I 1": lambda: _rand(3, 1, 7, 4, 6),
    "U 1": lambda: _rand(1, 500, 64, 50, 7),
    "U 17": lambda: _rand(17, 260, 20, 30, 8),
    "U 65": lambda: _rand(65, 260, 20, 30, 9),
    "E 256, N 128: the largest accepted": lambda: _rand(5, 300, 256, 128, 10, top=8),
}


def test_exact_cases_are_exact_in_fp32():
    """The float32 restatement of every exact case equals the float64 one."""
    for name, make in EXACT.items():
        u, v, N = make()
        i32, s32 = topn_ref(u, v, N, np.float32)
        i64, s64 = topn_ref(u, v, N)
        assert np.array_equal(i32, i64) and np.array_equal(s32.astype(np.float64), s64), name
        assert np.abs(u.astype(np.float64) @ v.astype(np.float64).T).max() < 2 ** 9 if len(v) else True


def test_float_case_is_well_conditioned():
    u, v = float_case()
    idx, score = topn_ref(u, v, 50, np.float32)
    check_float_rule(idx, score, u, v, 50, RTOL / 4, "float32 restatement")


# ------------------------------------------------------------------ CPU: the entry's checks
P = 0x1000  # a non-null pointer no check dereferences


def _call(user=P, us=8, U=4, item=P, is_=8, I=100, E=8, N=5, splits=1, oi=P, os_=P, ws=P, wsb=1 << 20):
    _lib.call("rs_topn_inner_product", user, us, U, item, is_, I, E, N, splits, oi, os_, ws, wsb, None)


def test_argument_checks_without_a_device():
    bad = [dict(user=None), dict(item=None), dict(oi=None), dict(os_=None), dict(U=-1), dict(I=-1), dict(us=7),
           dict(is_=7), dict(N=0), dict(N=-3), dict(E=0), dict(splits=-1), dict(E=8, N=129), dict(E=513, us=600, is_=600),
           dict(splits=2, ws=None), dict(splits=2, wsb=2 * 4 * 5 * 8 - 1), dict(splits=2, ws=P + 4),
           dict(I=1 << 31)]
    for kw in bad:
        with pytest.raises(_lib.RSError, match="rs_topn_inner_product"):
            _call(**kw)
    _call(U=0, user=None, item=None, oi=None, os_=None, ws=None, wsb=0)  # nothing to do: no launch, no error


def test_ok_bounds_and_workspace_size():
    ok, size = _lib.lib().rs_topn_inner_product_ok, _lib.lib().rs_topn_inner_product_workspace_size
    assert all(ok(E, N) for E in (1, 18, 32, 255, 256) for N in (1, 50, 127, 128))
    assert not ok(0, 5) and not ok(8, 0) and not ok(8, 129) and not ok(513, 1)
    assert ok(256, 128) and not ok(257, 128) and not ok(256, 129)   # the LDS budget at N 128, the list cap
    assert ok(320, 122) and not ok(320, 123) and ok(512, 26) and not ok(512, 27)
    assert retrieval.topn_ok(32, 50) and not retrieval.topn_ok(32, 200)
    sizes = [size(100, 5000, 50, s) for s in range(1, 80)]
    assert sizes[0] == 0 and sizes[1] == 2 * 100 * 50 * 8
    assert all(a <= b for a, b in zip(sizes, sizes[1:]))
    assert sizes[-1] == sizes[63] == 63 * 100 * 50 * 8   # clamped to 64: 313 tiles in splits of 5, none empty
    assert size(100, 100, 50, 1000) == 7 * 100 * 50 * 8                                     # ... and to the 7 tiles
    assert size(100, 5000, 50, 0) >= 0 and size(0, 0, 1, 0) == 0
    assert size(-1, 5, 5, 1) == -1 and size(5, -1, 5, 1) == -1 and size(5, 5, 0, 1) == -1 and size(5, 5, 5, -1) == -1


def test_host_api_errors():
    z = np.zeros
    with pytest.raises(ValueError, match="matrix"):
        rs.topn_inner_product(z(3, np.float32), z((2, 3), np.float32), 5)
    with pytest.raises(ValueError, match="user rows hold 3"):
        rs.topn_inner_product(z((2, 3), np.float32), z((2, 4), np.float32), 5)
    with pytest.raises(ValueError, match="N must be"):
        rs.topn_inner_product(z((2, 3), np.float32), z((2, 3), np.float32), 0)
    with pytest.raises(ValueError, match="item_splits"):
        rs.topn_inner_product(z((2, 3), np.float32), z((2, 3), np.float32), 5, item_splits=-1)
    with pytest.raises(ValueError, match="empty rows"):
        rs.topn_inner_product(z((2, 0), np.float32), z((2, 0), np.float32), 5)
    m, _, _ = small_model("cpu")
    with pytest.raises(ValueError, match="batch_size"):
        m.predict_user_embedding({"uid": np.arange(3)}, batch_size=0)
    for name in ("predict_user_embedding", "predict_item_embedding", "retrieve", "recall"):
        assert callable(getattr(rs.DSSM, name))


# ------------------------------------------------------------------ GPU: the kernel through the host API
@gpu_test
@pytest.mark.parametrize("name", list(EXACT))
def test_exact_cases_bitwise(gpu, name):
    u, v, N = EXACT[name]()
    ref = topn_ref(u, v, N, np.float32)
    for fused in (True, False):
        idx, score = rs.topn_inner_product(torch.as_tensor(u).to(gpu), torch.as_tensor(v).to(gpu), N, fused=fused)
        same_bits(idx.cpu().numpy(), score.cpu().numpy(), *ref, what=f"{name}, fused={fused}")
    idx, score = rs.topn_inner_product(u, v, N)   # host arrays, the default dispatch
    same_bits(idx.cpu().numpy(), score.cpu().numpy(), *ref, what=f"{name}, fused=None")


@gpu_test
def test_refused_shapes_raise_or_take_the_torch_path(gpu):
    rng = np.random.default_rng(11)
    for E, N in ((257, 128), (256, 129)):
        assert not retrieval.topn_ok(E, N)
        u, v = exact(rng, (3, E), 8), exact(rng, (140, E), 8)
        with pytest.raises(_lib.RSError, match="not supported"):
            rs.topn_inner_product(u, v, N, fused=True)
        idx, score = rs.topn_inner_product(u, v, N)   # fused=None: the torch composition
        same_bits(idx.cpu().numpy(), score.cpu().numpy(), *topn_ref(u, v, N, np.float32), what=f"refused E {E} N {N}")


@gpu_test
def test_empty_sides(gpu):
    for fused in (True, False):
        idx, score = rs.topn_inner_product(np.ones((3, 4), np.float32), np.ones((0, 4), np.float32), 5, fused=fused)
        assert idx.dtype == torch.int32 and (idx == -1).all() and tuple(idx.shape) == (3, 5)
        assert torch.isneginf(score).all() and tuple(score.shape) == (3, 5)
        idx, score = rs.topn_inner_product(np.ones((0, 4), np.float32), np.ones((7, 4), np.float32), 5, fused=fused)
        assert tuple(idx.shape) == (0, 5) and tuple(score.shape) == (0, 5)


@gpu_test
def test_float_inputs(gpu):
    u, v = float_case()
    for fused in (True, False):
        idx, score = rs.topn_inner_product(torch.as_tensor(u).to(gpu), torch.as_tensor(v).to(gpu), 50, fused=fused)
        check_float_rule(idx.cpu().numpy(), score.cpu().numpy(), u, v, 50, RTOL, f"U 300, I 3707, fused={fused}")


# ------------------------------------------------------------------ GPU: the entry itself (splits, layout, workspace)
def run_entry(gpu, u, v, N, splits=0, us=None, is_=None, item_offset=0, stream_graph=False):
    """rs_topn_inner_product on copies with the given row strides (the gaps
    hold NaN), the item matrix item_offset floats into its buffer, the
    workspace exactly workspace_size bytes of 0xA5."""
    U, E = u.shape
    I = len(v)
    us, is_ = us or E, is_ or E
    ub = torch.full((U, us), float("nan"), device=gpu)
    ub[:, :E] = torch.as_tensor(u).to(gpu)
    vb = torch.full((I * is_ + item_offset,), float("nan"), device=gpu)
    vb[item_offset:].view(I, is_)[:, :E] = torch.as_tensor(v).to(gpu)
    need = _lib.lib().rs_topn_inner_product_workspace_size(U, I, N, splits)
    ws = torch.full((max(need, 8),), 0xA5, dtype=torch.uint8, device=gpu)
    idx = torch.full((U, N), -7, dtype=torch.int32, device=gpu)
    score = torch.full((U, N), float("nan"), device=gpu)
    go = lambda: _lib.call("rs_topn_inner_product", ub.data_ptr(), us, U, vb.data_ptr() + 4 * item_offset, is_, I, E, N,  # noqa: E731
                           splits, idx.data_ptr(), score.data_ptr(), ws.data_ptr() if need else None, need,
                           _lib.stream())
    if not stream_graph:
        go()
        return idx.cpu().numpy(), score.cpu().numpy(), need
    go()
    eager = idx.clone(), score.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        go()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        go()
    for _ in range(2):
        idx.fill_(-7), score.fill_(float("nan")), ws.fill_(0x5A)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(idx, eager[0]) and torch.equal(score.view(torch.int32), eager[1].view(torch.int32))
    return idx.cpu().numpy(), score.cpu().numpy(), need


@gpu_test
def test_every_split_count_gives_the_same_bits(gpu):
    """I 100 = 7 tiles, N 50: with 7 splits every split holds fewer than N
    items; 9 and 1000 exceed the tile count (clamped); 0 = auto."""
    rng = np.random.default_rng(12)
    u, v = rng.integers(-1, 2, (37, 24)).astype(np.float32), rng.integers(-1, 2, (100, 24)).astype(np.float32)
    ref = topn_ref(u, v, 50, np.float32)
    needs = {}
    for s in (1, 2, 7, 0, 9, 1000):
        idx, score, needs[s] = run_entry(gpu, u, v, 50, splits=s)
        same_bits(idx, score, *ref, what=f"item_splits {s}")
    assert needs[1] == 0 and needs[2] == 2 * 37 * 50 * 8 and needs[7] == needs[9] == needs[1000] == 7 * 37 * 50 * 8
    # more than one round per split, ties across the split edges
    u, v, _ = EXACT["ties E32 (vector loads)"]()
    ref = topn_ref(u, v, 50, np.float32)
    for s in (1, 3, 0, 64):
        idx, score, _ = run_entry(gpu, u, v, 50, splits=s)
        same_bits(idx, score, *ref, what=f"ties, item_splits {s}")


@gpu_test
def test_strides_and_an_unaligned_item_pointer(gpu):
    rng = np.random.default_rng(13)
    u, v = exact(rng, (21, 32)), exact(rng, (333, 32))
    ref = topn_ref(u, v, 40, np.float32)
    for kw in (dict(us=40, is_=36), dict(us=33, is_=35), dict(item_offset=1), dict(item_offset=1, is_=37, splits=3)):
        idx, score, _ = run_entry(gpu, u, v, 40, **kw)
        same_bits(idx, score, *ref, what=str(kw))


@gpu_test
def test_graph_replay_gives_the_eager_bits(gpu):
    u, v, _ = EXACT["ties E18 (scalar loads)"]()
    for s in (1, 4):
        idx, score, _ = run_entry(gpu, u, v, 50, splits=s, stream_graph=True)
        same_bits(idx, score, *topn_ref(u, v, 50, np.float32), what=f"graph, item_splits {s}")


# ------------------------------------------------------------------ the model
N_ITEMS, N_USERS, T = 60, 20, 6


def small_model(device, seed=5):
    """Two sparse user features and one 'mean' var-len column, two item
    features, towers (16, 8); 60 items whose ids are a permutation of 1..60
    (position != id), 20 users."""
    rng = np.random.default_rng(seed)
    ucols = [S("uid", 40, 8), S("age", 9, 4), V(S("hist", N_ITEMS + 1, 8, embedding_name="movie_id"), T, "mean", "hist_len")]
    icols = [S("movie_id", N_ITEMS + 1, 8), S("genre", 7, 4)]
    sampler = rs.NegativeSampler("inbatch", 5, "movie_id", item_count=rng.integers(1, 50, N_ITEMS + 1).tolist())
    m = rs.DSSM(ucols, icols, user_dnn_hidden_units=(16, 8), item_dnn_hidden_units=(16, 8), sampler_config=sampler,
                seed=seed, device=device)
    L = rng.integers(1, T + 1, N_USERS)
    users = {"uid": rng.integers(0, 40, N_USERS), "age": rng.integers(0, 9, N_USERS),
             "hist": rng.integers(1, N_ITEMS + 1, (N_USERS, T)) * (np.arange(T)[None] < L[:, None]), "hist_len": L}
    items = {"movie_id": rng.permutation(N_ITEMS) + 1, "genre": rng.integers(0, 7, N_ITEMS)}
    return m, users, items


@gpu_test
@pytest.mark.parametrize("fused", [True, False])
def test_model_predict_retrieve_recall(gpu, fused):
    m, users, items = small_model(gpu)
    w = rand_weights(m, np.random.default_rng(6))
    m.set_keras_weights(w)
    u_ref = tower_ref(m, m.user_tower, "dnn", w, users)
    v_ref = tower_ref(m, m.item_tower, "dnn_1", w, items)
    u = m.predict_user_embedding(users, batch_size=7)     # 20 = 7 + 7 + 6
    v = m.predict_item_embedding(items, batch_size=16)    # 60 = 16 + 16 + 16 + 12
    assert_scaled_close(u, u_ref, what="predict_user_embedding")
    assert_scaled_close(v, v_ref, what="predict_item_embedding")
    assert torch.equal(u, m.user_embedding(users)) and torch.equal(v, m.predict_item_embedding(items))

    N = 10
    ids, score = m.retrieve(users, items, N=N, batch_size=7, fused=fused)
    assert ids.dtype == torch.int64 and tuple(ids.shape) == (N_USERS, N) and score.dtype == torch.float32
    pos_of = np.zeros(N_ITEMS + 1, np.int64)
    pos_of[items["movie_id"]] = np.arange(N_ITEMS)
    assert (items["movie_id"] != np.arange(N_ITEMS)).sum() > N_ITEMS // 2   # ids are not positions
    check_float_rule(pos_of[ids.cpu().numpy()].astype(np.int32), score.cpu().numpy(), u_ref, v_ref, N, RTOL, "retrieve")
    # a precomputed item matrix: positions, or the ids given
    pos, score2 = m.retrieve(users, v, N=N, fused=fused)
    assert np.array_equal(items["movie_id"][pos.cpu().numpy()], ids.cpu().numpy()) and torch.equal(score2, score)
    ids3, _ = m.retrieve(u, v, N=N, fused=fused, item_ids=items["movie_id"])
    assert torch.equal(ids3, ids)
    # N > items: padded with -1
    ids4, score4 = m.retrieve(users, items, N=N_ITEMS + 4, fused=fused)
    assert (ids4[:, N_ITEMS:] == -1).all() and torch.isneginf(score4[:, N_ITEMS:]).all()
    assert all(sorted(r) == sorted(items["movie_id"].tolist()) for r in ids4[:, :N_ITEMS].tolist())
    with pytest.raises(ValueError, match="item ids"):
        m.retrieve(u, v, N=N, item_ids=np.arange(5))

    # recall: every user's true item is its best one, except user 7's, which is its worst (rank 59 of 60)
    ref_pos, _ = topn_ref(u_ref, v_ref, N_ITEMS)
    true = items["movie_id"][ref_pos[:, 0]]
    assert m.recall(users, true, items, N=N, fused=fused) == 1.0
    true[7] = items["movie_id"][ref_pos[7, -1]]
    assert m.recall(users, true, items, N=N, fused=fused) == pytest.approx(19 / 20)
    per_user = [rs.recall_N([t], r, N) for t, r in zip(true.tolist(), ids.tolist())]
    assert m.recall(users, true, items, N=N, fused=fused) == pytest.approx(float(np.mean(per_user)))
