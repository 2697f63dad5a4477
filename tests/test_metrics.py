"""rs_binary_metrics / rs_auc and recommender_system_amd.metrics: log-loss,
accuracy, exact tie-aware ROC AUC and the impression-weighted group AUC.

The reference of every check is this file's numpy code: integer U2 (twice the
correctly ordered (positive, negative) pairs, a tie counting one), P, Q from
a stable argsort of the kernel's key map, fp64 loss terms, integer correct
counts.  The CPU part pins that reference against scikit-learn; the GPU part
asks for integers equal to it, auc bit-equal to U2 / (2 P Q), and the fp64
sums within 1e-12 relative (a term carries a few ulp of the fp64 log and the
sums are fixed trees: 1e-12 is orders above what arithmetic allows and orders
below any indexing mistake).
"""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

from recommender_system_amd import _lib, metrics

F32 = np.float32
TILE = 256 * 8  # pairs per radix-sort tile
SIZES = [1, 2, 63, 64, 65, TILE - 1, TILE, TILE + 1, 3 * TILE + 5]
GROUP_SIZES = [65, TILE + 1, 3 * TILE + 5]
SCORES = ["distinct", "equal", "levels", "mix"]
LABELS = ["random", "all_pos", "all_neg"]
EPS = 1e-7


# ------------------------------------------------------------- the reference
def key_map(scores):
    """Order-preserving uint32 key of fp32 scores; -0.0 ties with +0.0."""
    u = np.ascontiguousarray(scores, F32).view(np.uint32).copy()
    u[(u << np.uint32(1)) == 0] = 0
    return np.where(u >> np.uint32(31) == 1, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def ref_u2(scores, labels):
    """(U2, P, Q) as python ints."""
    if len(scores) == 0:
        return 0, 0, 0
    key = key_map(scores)
    order = np.argsort(key, kind="stable")
    k, y = key[order], labels[order] == 1
    head = np.r_[True, k[1:] != k[:-1]]
    rid = np.cumsum(head) - 1
    p_r = np.bincount(rid, y).astype(np.int64)
    n_r = np.bincount(rid, ~y).astype(np.int64)
    below = np.cumsum(n_r) - n_r
    return int(np.sum(p_r * (2 * below + n_r))), int(y.sum()), int((~y).sum())


def auc_of(U2, P, Q):
    return U2 / (2.0 * P * Q) if P and Q else float("nan")


def ref_gauc(scores, labels, groups):
    """(gauc, groups_used, impressions_used, terms); a term is size_g * AUC_g."""
    terms, used, imp = [], 0, 0
    for g in np.unique(groups):
        sel = groups == g
        U2, P, Q = ref_u2(scores[sel], labels[sel])
        if P and Q:
            terms.append(float(P + Q) * (U2 / (2.0 * P * Q)))
            used += 1
            imp += P + Q
    return (math.fsum(terms) / imp if imp else float("nan")), used, imp, terms


def ref_loss_terms(pred, labels):
    p, y = pred.astype(np.float64), labels.astype(np.float64)
    q = np.clip(p, EPS, 1.0 - EPS)
    return -(y * np.log(q + EPS) + (1.0 - y) * np.log(1.0 - q + EPS))


def ref_correct(pred, labels):
    return int(np.sum((pred > F32(0.5)) == (labels == 1)))


# ------------------------------------------------------------------ the cases
def make_scores(kind, N, rng):
    if kind == "distinct":
        return rng.permutation(N).astype(F32) * F32(0.37) - F32(N * 0.11)
    if kind == "equal":
        return np.full(N, 0.25, F32)
    if kind == "levels":
        return rng.choice(np.array([-1.5, -0.0, 0.0, 0.3, 2.0], F32), N)
    pool = np.array([-np.inf, -3.5, -1e-40, -1.4e-45, -0.0, 0.0, 1.4e-45, 1e-40, 2.0, np.inf], F32)
    s = np.where(rng.random(N) < 0.5, rng.choice(pool, N), rng.standard_normal(N).astype(F32)).astype(F32)
    s[:min(N, len(pool))] = pool[:min(N, len(pool))]
    return rng.permutation(s)


def make_labels(kind, N, rng):
    if kind == "all_pos":
        return np.ones(N, F32)
    if kind == "all_neg":
        return np.zeros(N, F32)
    y = (rng.random(N) < 0.3).astype(F32)
    if N >= 2:  # one positive and one negative forced
        i, j = rng.permutation(N)[:2]
        y[i], y[j] = 1.0, 0.0
    return y


def make_probs(N, rng):
    """fp32 probabilities with the clip ends and the threshold among them."""
    p = rng.random(N).astype(F32)
    special = np.array([0.0, 1.0, 0.5, np.nextafter(F32(0.5), F32(1)), 1e-8, 1 - 1e-8], F32)
    m = min(N, len(special))
    p[rng.permutation(N)[:m]] = special[:m]
    return p


@functools.lru_cache(maxsize=None)
def auc_case(N, skind, lkind):
    rng = np.random.default_rng([N, SCORES.index(skind), LABELS.index(lkind)])
    s, y = make_scores(skind, N, rng), make_labels(lkind, N, rng)
    s.setflags(write=False)
    y.setflags(write=False)
    return s, y, ref_u2(s, y)


@functools.lru_cache(maxsize=None)
def group_case(N, gkind):
    """scores (5 levels + noise on a third: ties inside groups), labels, dense
    int64 group ids, n_groups."""
    rng = np.random.default_rng([N, 77, ["one", "singletons", "random"].index(gkind)])
    s = make_scores("levels", N, rng)
    s = np.where(rng.random(N) < 0.35, rng.standard_normal(N).astype(F32), s).astype(F32)
    y = make_labels("random", N, rng)
    if gkind == "one":
        g, G = np.zeros(N, np.int64), 1
    elif gkind == "singletons":
        g, G = rng.permutation(N).astype(np.int64), N
    else:
        G = max(N // 7, 2)
        g = rng.integers(0, G, N).astype(np.int64)
        # one group wider than a sort tile where N allows, in scattered positions
        if N > 2 * TILE:
            g[rng.permutation(N)[:TILE + 300]] = 3
        y = np.where(g == 1, F32(0), y)  # a group without positives
    for a in (s, y, g):
        a.setflags(write=False)
    return s, y, g, G, ref_u2(s, y), ref_gauc(s, y, g)


# ------------------------------------------------------------------------ CPU
def test_key_map_orders_floats_and_ties_signed_zero():
    vals = np.array([-np.inf, -3.5, -1e-40, -1.4e-45, 0.0, 1.4e-45, 1e-40, 0.3, 2.0, np.inf], F32)
    k = key_map(vals).astype(np.int64)
    assert np.all(np.diff(k) > 0)
    assert key_map(np.array([-0.0], F32))[0] == key_map(np.array([0.0], F32))[0]


def test_issue_example():
    U2, P, Q = ref_u2(np.array([0.0, -0.0, 1.0, -1.0], F32), np.array([1, 0, 0, 1], F32))
    assert (U2, P, Q) == (1, 2, 2) and auc_of(U2, P, Q) == 0.125


@pytest.mark.parametrize("N", SIZES)
def test_reference_auc_matches_sklearn(N):
    """The integer formula == sklearn.metrics.roc_auc_score on every score
    pattern (to fp64 rounding: 1e-14).  The mix holds +-inf, which sklearn
    refuses, so it is ranked first: AUC depends on the order alone."""
    from sklearn.metrics import roc_auc_score
    checked = 0
    for skind in SCORES:
        s, y, (U2, P, Q) = auc_case(N, skind, "random")
        if not (P and Q):
            continue
        x = key_map(s).astype(np.float64) if skind == "mix" else s.astype(np.float64)
        assert abs(auc_of(U2, P, Q) - roc_auc_score(y, x)) <= 1e-14, skind
        checked += 1
    assert checked == (len(SCORES) if N >= 2 else 0)
    for lkind in ("all_pos", "all_neg"):
        assert math.isnan(auc_of(*auc_case(N, "distinct", lkind)[2]))


@pytest.mark.parametrize("N", GROUP_SIZES)
def test_reference_gauc_matches_per_group_sklearn(N):
    from sklearn.metrics import roc_auc_score
    s, y, g, G, _, (gauc, used, imp, terms) = group_case(N, "random")
    assert used >= 2 and used < len(np.unique(g)), "the case needs groups of both kinds"
    num = den = 0.0
    for gid in np.unique(g):
        sel = g == gid
        if 0 < y[sel].sum() < sel.sum():
            num += sel.sum() * roc_auc_score(y[sel], s[sel].astype(np.float64))
            den += sel.sum()
    assert den == imp and abs(gauc - num / den) <= 1e-13
    assert group_case(N, "singletons")[5][1:3] == (0, 0) and math.isnan(group_case(N, "singletons")[5][0])
    one = group_case(N, "one")
    assert one[5][1:3] == (1, N) and abs(one[5][0] - auc_of(*one[4])) <= 1e-15


def test_reference_loss_and_accuracy_match_sklearn():
    """Keras' form log(clip(p) + 1e-7) differs from sklearn's log(clip(p)) by
    at most 1e-7 / p per term: below 1.1e-5 for p in [0.01, 0.99]."""
    from sklearn.metrics import accuracy_score, log_loss
    rng = np.random.default_rng(5)
    for N in SIZES[2:]:
        p = (0.01 + 0.98 * rng.random(N)).astype(F32)
        y = make_labels("random", N, rng)
        mine = math.fsum(ref_loss_terms(p, y)) / N
        assert abs(mine - log_loss(y, p.astype(np.float64), labels=[0, 1])) <= 1.1e-5
        assert ref_correct(p, y) == round(accuracy_score(y, (p > 0.5).astype(F32)) * N)


def test_argument_validation_without_device():
    lib, one = _lib.lib(), C.c_void_p(1)
    assert lib.rs_binary_metrics_workspace_size(1 << 31) == -1
    assert lib.rs_binary_metrics_workspace_size(-1) == -1
    assert lib.rs_binary_metrics_workspace_size((1 << 31) - 1) > 0
    assert lib.rs_auc_workspace_size(1 << 31, 0) == -1
    assert lib.rs_auc_workspace_size(10, -1) == -1
    assert lib.rs_auc_workspace_size(-1, 0) == -1
    assert lib.rs_auc_workspace_size(10, 4) > lib.rs_auc_workspace_size(10, 0) > 0
    assert lib.rs_binary_metrics(None, 1, None, 4, 0, None, None, None) == -1
    assert b"null" in lib.rs_last_error_string()
    assert lib.rs_binary_metrics(one, 1, one, 4, 0, None, one, None) == -1
    assert lib.rs_binary_metrics(one, 1, one, -1, 0, one, one, None) == -1
    assert lib.rs_binary_metrics(one, 1, one, 1 << 31, 0, one, one, None) == -1
    assert lib.rs_binary_metrics(one, 0, one, 4, 0, one, one, None) == -1
    assert lib.rs_auc(None, 1, None, None, 0, 0, 4, None, None, None) == -1
    assert b"null" in lib.rs_last_error_string()
    assert lib.rs_auc(one, 1, one, None, 0, 0, -1, one, one, None) == -1
    assert lib.rs_auc(one, 1, one, None, 0, 0, 1 << 31, one, one, None) == -1
    assert lib.rs_auc(one, 1, one, one, _lib.ID_I32, 0, 4, one, one, None) == -1
    assert b"n_groups" in lib.rs_last_error_string()
    assert lib.rs_auc(one, 1, one, one, _lib.ID_F32, 3, 4, one, one, None) == -1


def test_cpu_tensor_raises():
    p, y = torch.rand(8), torch.zeros(8)
    for fn in (lambda: metrics.binary_metrics(p, y), lambda: metrics.roc_auc(p, y),
               lambda: metrics.group_auc(p, y, torch.zeros(8, dtype=torch.int64), 1),
               lambda: metrics.BinaryMetrics("cpu").update(p, y)):
        with pytest.raises(_lib.RSError, match="device"):
            fn()


# ------------------------------------------------------------------------ GPU
def _dev(a, gpu):
    return torch.as_tensor(np.array(a), device=gpu)  # (a copy: the cached cases are read-only)


def _same(a, b):
    return a == b or (isinstance(a, float) and math.isnan(a) and math.isnan(b))


@pytest.mark.gpu
@pytest.mark.parametrize("N", SIZES)
def test_auc_exact(gpu, N):
    """U2, P, Q equal the reference as integers and auc is bit-equal to the
    same fp64 expression, for every score and label pattern."""
    for skind in SCORES:
        for lkind in LABELS:
            s, y, (U2, P, Q) = auc_case(N, skind, lkind)
            got = metrics.auc_stats(_dev(s, gpu), _dev(y, gpu))
            what = f"N={N} {skind} {lkind}"
            assert (got["u2"], got["n_pos"], got["n_neg"], got["n"]) == (U2, P, Q, N), what
            assert _same(got["auc"], auc_of(U2, P, Q)), what
            if lkind != "random" or N == 1:
                assert math.isnan(got["auc"]), what
    s, y, _ = auc_case(N, "mix", "random")
    assert _same(metrics.roc_auc(_dev(s, gpu), _dev(y, gpu)), auc_of(*ref_u2(s, y)))


@pytest.mark.gpu
def test_issue_example_on_device(gpu):
    got = metrics.auc_stats(_dev(np.array([0.0, -0.0, 1.0, -1.0], F32), gpu), _dev(np.array([1, 0, 0, 1], F32), gpu))
    assert (got["u2"], got["n_pos"], got["n_neg"], got["auc"]) == (1, 2, 2, 0.125)


@pytest.mark.gpu
@pytest.mark.parametrize("N", SIZES)
def test_binary_metrics(gpu, N):
    """loss within 1e-12 relative of the fp64 reference on the same fp32
    probabilities (0.0, 1.0, 0.5 among them), integer counts equal, auc
    bit-equal; a [N, 1] column of a wider matrix (stride 3) gives the same
    words; a second call is bit-identical."""
    for lkind in LABELS:
        rng = np.random.default_rng([N, 9, LABELS.index(lkind)])
        p, y = make_probs(N, rng), make_labels(lkind, N, rng)
        U2, P, Q = ref_u2(p, y)
        loss_sum = math.fsum(ref_loss_terms(p, y))
        got = metrics.binary_metrics(_dev(p, gpu), _dev(y, gpu))
        what = f"N={N} {lkind}"
        assert (got["n"], got["n_pos"], got["n_neg"], got["u2"]) == (N, P, Q, U2), what
        assert got["n_correct"] == ref_correct(p, y), what
        assert got["accuracy"] == ref_correct(p, y) / N, what
        assert abs(got["loss_sum"] - loss_sum) <= 1e-12 * abs(loss_sum), (what, got["loss_sum"], loss_sum)
        assert abs(got["loss"] - loss_sum / N) <= 1e-12 * abs(loss_sum / N), what
        assert _same(got["auc"], auc_of(U2, P, Q)), what
        wide = torch.zeros(N, 3, device=gpu)
        wide[:, 1] = _dev(p, gpu)
        again = metrics.binary_metrics(wide[:, 1:2], _dev(y, gpu).reshape(N, 1))
        assert all(_same(got[k], again[k]) for k in got) and set(got) == set(again), what


@pytest.mark.gpu
@pytest.mark.parametrize("N", [65, 3 * TILE + 5])
def test_accumulate_three_ragged_pieces(gpu, N):
    rng = np.random.default_rng([N, 11])
    p, y = make_probs(N, rng), make_labels("random", N, rng)
    whole = metrics.binary_metrics(_dev(p, gpu), _dev(y, gpu))
    cuts = [0, N // 5, N // 5 + N // 2 + 1, N]
    acc = metrics.BinaryMetrics(gpu)
    for a, b in zip(cuts[:-1], cuts[1:]):
        acc.update(_dev(p[a:b], gpu), _dev(y[a:b], gpu))
    got = acc.result()
    for k in ("n", "n_pos", "n_neg", "n_correct", "u2", "accuracy"):
        assert got[k] == whole[k], k
    assert got["auc"] == whole["auc"]
    ref = math.fsum(ref_loss_terms(p, y))
    assert abs(got["loss_sum"] - ref) <= 1e-12 * abs(ref), (got["loss_sum"], ref)
    # rs_binary_metrics itself: accumulate into a zeroed result
    res = torch.zeros(8, dtype=torch.int64, device=gpu)
    pd, yd = _dev(p, gpu), _dev(y, gpu)
    ws = torch.empty(_lib.lib().rs_binary_metrics_workspace_size(N), dtype=torch.uint8, device=gpu)
    for a, b in zip(cuts[:-1], cuts[1:]):
        _lib.call("rs_binary_metrics", pd[a:b].data_ptr(), 1, yd[a:b].data_ptr(), b - a, 1, res.data_ptr(),
                  ws.data_ptr(), _lib.stream())
    w = res.tolist()
    assert w[:3] == [N, whole["n_pos"], whole["n_correct"]] and w[4:] == [0, 0, 0, 0]
    assert metrics._f64(w[3]) == got["loss_sum"]


@pytest.mark.gpu
@pytest.mark.parametrize("N", GROUP_SIZES)
@pytest.mark.parametrize("gkind", ["one", "singletons", "random"])
def test_group_auc(gpu, N, gkind):
    s, y, g, G, (U2, P, Q), (gauc, used, imp, terms) = group_case(N, gkind)
    if gkind == "random":
        assert used >= 2, "the case must not pass vacuously"
    for dtype in (np.int64, np.int32):
        got = metrics.auc_stats(_dev(s, gpu), _dev(y, gpu), _dev(g.astype(dtype), gpu), G)
        assert (got["u2"], got["n_pos"], got["n_neg"]) == (U2, P, Q)
        assert _same(got["auc"], auc_of(U2, P, Q))
        assert (got["groups_used"], got["impressions_used"]) == (used, imp)
        if used:
            assert abs(got["gauc"] - gauc) <= 1e-12 * abs(gauc), (got["gauc"], gauc)
        else:
            assert math.isnan(got["gauc"])
    again = metrics.auc_stats(_dev(s, gpu), _dev(y, gpu), _dev(g, gpu), G)
    assert all(_same(got[k], again[k]) for k in got), "repeated calls are bit-identical"
    assert _same(metrics.group_auc(_dev(s, gpu), _dev(y, gpu), _dev(g, gpu)), got["gauc"])  # n_groups from the ids
    full = metrics.binary_metrics(torch.sigmoid(_dev(s, gpu)), _dev(y, gpu), _dev(g, gpu), G)
    assert {"loss", "accuracy", "auc", "n", "n_pos", "gauc", "groups_used", "impressions_used"} <= set(full)
    if gkind == "one":
        assert abs(got["gauc"] - got["auc"]) <= 1e-15


@pytest.mark.gpu
def test_bad_inputs_raise(gpu):
    N = 70
    rng = np.random.default_rng(3)
    p, y = make_probs(N, rng), make_labels("random", N, rng)
    g = rng.integers(0, 5, N)
    for bad in (5, -1, 1 << 40):
        gb = g.copy()
        gb[17] = bad
        with pytest.raises(_lib.BadIdError):
            metrics.group_auc(_dev(p, gpu), _dev(y, gpu), _dev(gb, gpu), 5)
    pn = p.copy()
    pn[3] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        metrics.binary_metrics(_dev(pn, gpu), _dev(y, gpu))
    with pytest.raises(ValueError, match="NaN"):
        metrics.roc_auc(_dev(pn, gpu), _dev(y, gpu))
    yb = y.copy()
    yb[5] = 0.5
    with pytest.raises(ValueError, match="neither 0 nor 1"):
        metrics.binary_metrics(_dev(p, gpu), _dev(yb, gpu))
    with pytest.raises(ValueError, match="neither 0 nor 1"):
        metrics.roc_auc(_dev(p, gpu), _dev(yb, gpu))
    ok = metrics.binary_metrics(_dev(p, gpu), _dev(y, gpu), _dev(g, gpu), 5)  # nothing sticks
    assert ok["n"] == N and not math.isnan(ok["auc"])
