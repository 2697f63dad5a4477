"""The row-sharded exchange (shard.hip, shard_route.hpp, shard_fm.hip, shard_dedup.hip, rs_shard_owner_fm_grad of
dnn_train.hip, rs_rows_fm_fwd), one entry point at a time through the C ABI, against plain numpy int64 / float64
restatements, at every shape where a launcher or a kernel takes another branch.  The Sharded* classes stay with
tests/test_sharded_gloo.py.

Part A (CPU): the references are pinned to CpuOps of tests/test_sharded_gloo.py (integers exactly, float64 within
1e-12) and to np.add.at; the launchers' dispatch (dh_per_field, dh_n2 / LW, the chunk of dedup_scatter_f, seg_chunk,
the kernels of rs_gather_rows / rs_unpermute_rows with their alignment condition, launch_pipe_kv, the constant shape
of launch_pipe4, fm_geom, rs_fm_partial_width) is restated in Python, so every GPU case below is (shape) -> the name
of the branch it takes, computed and not typed, and every branch is named by a case; every entry is called with dummy
pointers on both sides of every bound of its RS_REQUIRE lines; and every GPU case with floating-point output is
conditioned: the same restatement in float32 numpy sits within a quarter of the GPU tolerance of the float64 one.

Part B (GPU): ids as int32 / int64 / float32, id_stride = n_fields or n_fields + 3 with garbage in the padding,
stored outputs prefilled with a sentinel or NaN, padding words checked unchanged, every call twice on fresh outputs
for bitwise equality, a clean run (flag 0) and a run with out-of-range ids (too large, -1, NaN for float32: flag
raised, every other lookup's result unchanged), err_flag = NULL where flag_error allows it.

A bad id, as rs_capi.h states it: rs_shard_bucketize keeps it as a lookup of owner 0 with send word -1 (perm stays a
permutation); rs_shard_slot_bucketize gives it no rank, no position and no part of counts (before this file it was
ranked and counted as owner 0's and could push a valid lookup past cap: test_slot_bucketize pins the fix).

Inputs keep the references O(1), as tests/test_fused_forwards.py draws them: rows N(0,1) * 0.5, dense U[0,1), FM v
N(0,1) / sqrt(d), w1 N(0,1) / sqrt(d).  Tolerances are the project's: integers and copied rows exact; partial
records, s columns and drows: helpers.assert_scaled_close at 1e-5; the logit, dw1, dv and a dedup gradient row
(sums that cancel or run over many lookups): |err| <= SUM_TOL * sum |terms|, sum |terms| from the reference run on
absolute values; g and the loss of rs_shard_fm_combine_grad from the logit's bound delta: |dg| <= grad_scale *
delta / 4 + 1e-5 |g| (sigmoid' <= 1/4), |dloss| <= delta + 1e-5 |loss| (|dBCE/dz| <= 1).
"""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

from recommender_system_amd import _lib
from tests.helpers import RTOL, assert_scaled_close
from tests.test_fused_forwards import KINDS, fm_geom, ref_fm
from tests.test_sharded_gloo import CpuOps
from tests.test_train_blocks import F32, F64, SENT, SUM_TOL, _d, _dev, _nrm, _p, _refused, _twice

torch = pytest.importorskip("torch")

I32, I64 = np.int32, np.int64
ISENT = -7777  # integer outputs are prefilled with it
KIND_OF = {np.dtype(t): kd for t, kd in KINDS}
DTYPES = (np.int32, np.int64, np.float32)


# --------------------------------------------------------------------------
# Layouts and ids
# --------------------------------------------------------------------------
def layout(vocab, world, rpr=None, offs=None):
    """The concatenated table's fields, the block split (rows_per_rank) and each owner's field range."""
    vocab = np.asarray(vocab, I64)
    offs = np.concatenate([[0], np.cumsum(vocab)[:-1]]).astype(I64) if offs is None else np.asarray(offs, I64)
    total = int((offs + vocab).max())
    rpr = -(-total // world) if rpr is None else int(rpr)
    of = []
    for o in range(world):
        lo_r, hi_r = o * rpr, min(total, (o + 1) * rpr)
        cs = [c for c in range(len(vocab)) if offs[c] < hi_r and offs[c] + vocab[c] > lo_r]
        of.append((cs[0], len(cs)) if cs else (0, 0))
    return SimpleNamespace(vocab=vocab, offs=offs, F=len(vocab), world=world, rpr=rpr, total=total,
                           owner_fields=np.asarray(of, I32), slot_stride=max(1, max(n for _, n in of)))


def decode(ids, vocab):
    """Ids<KIND>::decode: (valid [B, F], id int64, 0 where invalid).  float32: valid when f > -1 and f < vocab, then
    trunc(f); NaN is invalid."""
    ids, vocab = np.asarray(ids), np.asarray(vocab, I64)[None, :]
    if ids.dtype == np.float32:
        f = ids.astype(F64)
        with np.errstate(invalid="ignore"):
            ok = (f > -1.0) & (f < vocab.astype(F64))
        return ok, np.trunc(np.where(ok, f, 0.0)).astype(I64)
    v = ids.astype(I64)
    ok = (v >= 0) & (v < vocab)
    return ok, np.where(ok, v, 0)


def rows_of(ids, L):
    """(valid, global row, owner, local row) of every lookup, flat in lookup order j = b * F + c."""
    ok, idv = decode(ids, L.vocab)
    row = L.offs[None, :] + idv
    owner = np.minimum(row // L.rpr, L.world - 1)
    return ok.reshape(-1), row.reshape(-1), owner.reshape(-1), (row - owner * L.rpr).reshape(-1)


def with_bad(ids, vocab, rng, count=3):
    """A copy of ids with `count` lookups out of range: too large, -1, and for float32 NaN.  (ids, bad mask)."""
    ids = np.array(ids)
    B, F = ids.shape
    pos = rng.choice(B * F, size=min(count, B * F), replace=False)
    for i, p in enumerate(pos):
        b, c = divmod(int(p), F)
        v = int(vocab[c])
        if ids.dtype == np.float32:
            big = np.float32(v)  # the first float32 that is >= vocab
            big = big if float(big) >= v else np.nextafter(big, np.float32(np.inf))
            ids[b, c] = (big, np.float32(-1.0), np.float32(np.nan))[i % 3]
        else:
            ids[b, c] = (min(v, np.iinfo(ids.dtype).max), -1, min(v + 5, np.iinfo(ids.dtype).max))[i % 3]
    bad = np.zeros(B * F, bool)
    bad[pos] = True
    assert not decode(ids, vocab)[0].reshape(-1)[pos].any()
    return ids, bad


def random_ids(rng, B, vocab, dtype=I64, hot=0.0):
    """ids [B, F] in range; hot: the share of lookups that repeat one of a field's first 3 ids."""
    vocab = np.asarray(vocab, I64)
    ids = np.stack([rng.integers(0, v, B) for v in vocab], 1)
    if hot:
        ids = np.where(rng.random(ids.shape) < hot, rng.integers(0, 3, ids.shape) % vocab[None, :], ids)
    return ids.astype(dtype)


# --------------------------------------------------------------------------
# References (int64 / float64; dt = float32: the conditioning run)
# --------------------------------------------------------------------------
def ref_bucketize(ids, L):
    """rs_shard_bucketize: (counts, perm, send_rows), stable owner-major; a bad id is owner 0's with send word -1."""
    ok, row, owner, local = rows_of(ids, L)
    owner, local = np.where(ok, owner, 0), np.where(ok, local, -1)
    order = np.argsort(owner, kind="stable")
    perm = np.empty_like(order)
    perm[order] = np.arange(order.size)
    send = np.empty(order.size, I64)
    send[perm] = local
    return np.bincount(owner, minlength=L.world), perm, send


def ref_slot_bucketize(ids, L, cap, send=None):
    """rs_shard_slot_bucketize: (counts, slot_of, send, overflow).  The valid lookups of owner o take ranks 0, 1, ..
    in lookup order; rank r < cap -> slot o * cap + r; a bad id takes nothing; unused send words keep their content."""
    ok, row, owner, local = rows_of(ids, L)
    slot = np.full(ok.size, -1, I64)
    send = np.full(L.world * cap, -1, I64) if send is None else np.array(send, I64)
    counts = np.zeros(L.world, I64)
    over = False
    for o in range(L.world):
        idx = np.nonzero(ok & (owner == o))[0]
        counts[o] = idx.size
        over |= idx.size > cap
        idx = idx[:cap]
        slot[idx] = o * cap + np.arange(idx.size)
        send[o * cap + np.arange(idx.size)] = local[idx]
    return counts, slot, send, over


def ref_field_route(ids, L, slot_stride):
    """rs_shard_field_route / _row_route: (send [world, B, slot_stride], slot_of [B, F])."""
    ok, idv = decode(ids, L.vocab)
    B = ok.shape[0]
    out = np.full((L.world, B, slot_stride), -1, I64)
    slot = np.full((B, L.F), -1, I64)
    row = L.offs[None, :] + idv
    for o, (lo, n) in enumerate(L.owner_fields):
        for j in range(n):
            loc = row[:, lo + j] - o * L.rpr
            m = ok[:, lo + j] & (loc >= 0) & (loc < L.rpr)
            out[o, m, j] = loc[m]
            slot[m, lo + j] = (o * B + np.nonzero(m)[0]) * slot_stride + j
    return out, slot


def ref_dedup_route(ids, L, cap, order):
    """rs_shard_dedup_route: (send, slot_of, overflow).  order "row": an owner's distinct rows in row order (the
    sort path); "first": field by field, inside a field in order of first occurrence (the per-field hash path)."""
    ok, row, owner, local = rows_of(ids, L)
    send, slot, over = np.full(L.world * cap, -1, I64), np.full(ok.size, -1, I64), False
    for o in range(L.world):
        idx = np.nonzero(ok & (owner == o))[0]
        if not idx.size:
            continue
        if order == "first":
            idx = idx[np.lexsort((idx // L.F, idx % L.F))]  # field-major, lookup order inside a field
        ur, first, inv = np.unique(row[idx], return_index=True, return_inverse=True)
        rank = np.argsort(np.argsort(first)) if order == "first" else np.arange(ur.size)
        u = rank[inv]
        over |= ur.size > cap
        keep = u < cap
        slot[idx[keep]] = o * cap + u[keep]
        send[o * cap + u[keep]] = row[idx[keep]] - o * L.rpr
    return send, slot, over


def check_dedup_route(ids, L, cap, send, slot_of):
    """What the header promises whatever the numbering: owner o's words [0, n_o) are n_o = min(distinct, cap)
    distinct local rows it owns, the rest -1; every valid lookup's slot holds its own row (-1 only past the
    capacity); a bad id has slot -1 and takes no send word.  Returns overflow."""
    ok, row, owner, local = rows_of(ids, L)
    send, slot = np.asarray(send, I64), np.asarray(slot_of, I64).reshape(-1)
    assert np.all(slot[~ok] == -1)
    over = False
    for o in range(L.world):
        mine = ok & (owner == o)
        need = np.unique(row[mine])
        n_o = min(need.size, cap)
        words = send[o * cap:(o + 1) * cap]
        assert np.all(words[n_o:] == -1), o
        got = words[:n_o] + o * L.rpr
        assert np.unique(got).size == n_o and np.isin(got, need).all(), o
        over |= need.size > cap
        good = slot[mine] >= 0
        assert need.size > cap or good.all(), o
        s = slot[mine][good]
        assert np.all(s // cap == o)
        np.testing.assert_array_equal(send[s] + o * L.rpr, row[mine][good])
    return over


def ref_dedup_grad(grad, slot_of, n_slots, dt=F64, ab=False):
    """rs_shard_dedup_grad: dst[slot] = the sum of the gradient rows of the slot's lookups; (dst, written)."""
    slot = np.asarray(slot_of, I64).reshape(-1)
    g = np.asarray(grad, dt).reshape(slot.size, -1)
    g = np.abs(g) if ab else g
    dst = np.zeros((n_slots, g.shape[1]), dt)
    np.add.at(dst, slot[slot >= 0], g[slot >= 0])
    return dst, np.isin(np.arange(n_slots), slot[slot >= 0])


def ref_gather(table, rows, n_rows):
    """rs_gather_rows: (out, flag): row -1 a zero row, any other row outside [0, n_rows) a zero row and the flag."""
    rows = np.asarray(rows, I64)
    inr = (rows >= 0) & (rows < n_rows)
    out = np.where(inr[:, None], np.asarray(table)[np.where(inr, rows, 0)], 0)  # (+0: a zero row, bit for bit)
    return out, int(np.any(~inr & (rows != -1)))


def ref_scatter(src, slot_of, k, dst):
    """rs_scatter_rows: dst[slot_of[j]] = lookup j's k floats of src [B, >= F * k] (slot < 0 skipped)."""
    slot = np.asarray(slot_of, I64).reshape(-1)
    F = slot.size // src.shape[0]
    rows = np.asarray(src)[:, :F * k].reshape(-1, k)
    dst = np.array(dst)
    dst[slot[slot >= 0]] = rows[slot >= 0]
    return dst


def ref_owner_fm(recv, lo, n_owned, shard, shard_rows, nd, k, w1, v, kfm, dt=F64, ab=False):
    """rs_shard_owner_fm: records [s_0 .. s_{kfm-1}, x @ w1, sum x^2 |v|^2] over the owned fields; a local row
    outside [0, shard_rows) contributes 0 (and, unless it is -1, raises the flag).  (records [n_pairs, kfm + 2],
    flag)"""
    f = np.abs if ab else (lambda t: t)
    recv = np.asarray(recv, I64)
    T, w1, v = f(np.asarray(shard, dt)), f(np.asarray(w1, dt).reshape(-1)), f(np.asarray(v, dt))
    res = np.zeros((recv.shape[0], kfm + 2), dt)
    flag = 0
    for j in range(n_owned):
        e = nd + (lo + j) * k + np.arange(k)
        loc = recv[:, j]
        inr = (loc >= 0) & (loc < shard_rows)
        flag |= int(np.any(~inr & (loc != -1)))
        x = np.zeros((recv.shape[0], k), dt)
        x[inr] = T[loc[inr]]
        res[:, :kfm] += x @ v[e]
        res[:, kfm] += x @ w1[e]
        res[:, kfm + 1] += (x * x) @ (v[e] ** 2).sum(1)
    return res, flag


def ref_combine(part, dense, nd, w0, w1, v, kfm, dt=F64, ab=False):
    """rs_shard_fm_combine on partial records part [world, B, >= kfm + 2]: (logit, s [B, kfm]); ab: (sum |terms|, -)."""
    f = np.abs if ab else (lambda t: t)
    p = f(np.asarray(part, dt)).sum(0)
    d = f(np.asarray(dense, dt).reshape(p.shape[0], -1)[:, :nd])
    w1, v, w0 = f(np.asarray(w1, dt).reshape(-1)), f(np.asarray(v, dt)), f(dt(np.asarray(w0).reshape(-1)[0]))
    S = p[:, :kfm] + d @ v[:nd]
    lin = p[:, kfm] + d @ w1[:nd]
    q = p[:, kfm + 1] + (d * d) @ (v[:nd] ** 2).sum(1)
    sgn = dt(1.0 if ab else -1.0)
    return lin + w0 + dt(0.5) * ((S ** 2).sum(1) + sgn * q), S


def ref_bce(z, t, scale, dt=F64):
    """(g, loss) of rs_shard_fm_combine_grad from the logit."""
    z, t = np.asarray(z, dt), np.asarray(t, dt)
    return (1 / (1 + np.exp(-z)) - t) * dt(scale), np.maximum(z, 0) - z * t + np.log1p(np.exp(-np.abs(z)))


def ref_owner_rows(recv, n_owned, shard, shard_rows, k, dt=F64):
    """rows_ws of rs_shard_owner_fm_grad: [n_pairs, n_owned * k], an absent row 0."""
    recv = np.asarray(recv, I64)[:, :n_owned]
    inr = (recv >= 0) & (recv < shard_rows)
    x = np.where(inr[:, :, None], np.asarray(shard, dt)[np.where(inr, recv, 0)], 0)
    return x.reshape(recv.shape[0], n_owned * k)


# --------------------------------------------------------------------------
# The launchers' dispatch, restated (shard.hip, shard_dedup.hip, rs_common.hpp, shard_fm.hip)
# --------------------------------------------------------------------------
DH_MAXB, DD_MAXF, DH_MAXW = 4096, 1024, 4096


def dh_per_field(batch, F, world):
    return batch <= DH_MAXB and F <= DD_MAXF and world <= DH_MAXW


def dh_n2(batch):
    N2 = 1024
    while N2 < batch:
        N2 <<= 1
    return N2


def dh_lw(batch):
    return {1024: 0, 2048: 1, 4096: 2}[dh_n2(batch)]


def dedup_route_branch(batch, F, world):
    """rs_shard_dedup_route: the sort path, or dedup_field_hash<KIND, LW> and the chunk of dedup_scatter_f."""
    if not dh_per_field(batch, F, world):
        return "sort"
    return f"hash LW={dh_lw(batch)} chunk={(F + 255) // 256}"


def seg_chunk(W):
    c = 256
    while c < 4 * W:
        c <<= 1
    return c


def dedup_grad_branch(batch, F, world, k):
    """rs_shard_dedup_grad: the grouping launch, seg_chunk and whether dedup_grad_cross runs."""
    n, ch = batch * F, seg_chunk(k)
    group = f"dedup_group_f<{dh_lw(batch)}>" if dh_per_field(batch, F, world) else "sorted"
    return f"{group} C={ch} {'piece+cross' if (n + ch - 1) // ch > 1 else 'piece'}"


def gather_branch(k, n, table_off=0, out_off=0):
    """rs_gather_rows: table_off / out_off = the pointers' byte offsets from a 16-B boundary."""
    al = table_off % 16 == 0 and out_off % 16 == 0
    if k == 16 and n < (1 << 29) and al:
        return "gather_rows_k16"
    return "gather_rows_kernel<4>" if k % 4 == 0 and al else "gather_rows_kernel<1>"


def unpermute_branch(k, src_off=0, dst_off=0):
    return "unpermute_rows_kernel<4>" if k % 4 == 0 and src_off % 16 == 0 and dst_off % 16 == 0 else \
        "unpermute_rows_kernel<1>"


def partial_width(kfm):
    return -1 if kfm < 1 else (kfm + 2 + 3) // 4 * 4


def pipe_branch(nd, n_fields, k, kfm, n_owned):
    """launch_pipe_kv / launch_pipe4 for an owner part over n_owned fields (the combine alone: n_owned = 0): the
    instantiation shard_fm_pipe<KV, NT, NW, MC> (+ FC, KFMC at the constant shape).  The owner's EmbedFmArgs carries
    nd = 0 whatever the model's nd (the requester adds the dense block), so the constant shape is n_owned 26,
    kfm 10, k 16."""
    g = fm_geom(nd, n_fields, k, kfm)
    assert g["mfma"]
    KV, NT = g["KV"], g["NT"]
    if NT == 1:
        nw, mc = (4, 1) if n_owned <= 4 else ((8, 1) if n_owned <= 8 else ((16, 1) if n_owned <= 32 else (16, 0)))
    else:
        NT, (nw, mc) = 2, ((16, 1) if n_owned <= 32 else (16, 0))
    if (KV, NT, nw, mc) == (4, 1, 16, 1) and n_owned == 26 and kfm == 10:
        return "shard_fm_pipe<4,1,16,1,26,10>"
    return f"shard_fm_pipe<{KV},{NT},{nw},{mc}>"


def pipe_line(name):
    """The launch_pipe_kv line (NT, NW, MC) of an instantiation's name, "const" for launch_pipe4's constant shape."""
    t = name[name.index("<") + 1:-1].split(",")
    return "const" if len(t) == 6 else ",".join(t[1:])


PIPE_LINES = {"1,4,1", "1,8,1", "1,16,1", "1,16,0", "2,16,1", "2,16,0", "const"}


# --------------------------------------------------------------------------
# Cases.  Every case is plain data: the CPU part computes its branch and conditions it, the GPU part runs it.
# --------------------------------------------------------------------------
RPR_MAX = (1 << 31) - 1


def boundary_case(rpr, world, F, B, dtype, seed=0):
    """Fields laid as windows over the rows o * rpr - 1, o * rpr, o * rpr + 1 of every owner boundary (a routing
    kernel never touches a table, so a huge offset costs nothing); sample b of field c asks for the window's
    targets in turn, so B >= a window's targets reaches all of them.  (layout, ids [B, F] of dtype)"""
    t = sorted({r for o in range(world + 1) for r in (o * rpr - 1, o * rpr, o * rpr + 1) if 0 <= r < world * rpr})
    assert len(t) >= F, (rpr, world, F)
    groups = np.array_split(np.asarray(t, I64), F)
    offs, vocab = [int(g[0]) for g in groups], [int(g[-1] - g[0] + 1) for g in groups]
    assert max(vocab) <= {np.dtype(np.int32): RPR_MAX, np.dtype(np.int64): 1 << 62, np.dtype(np.float32): 1 << 24}[
        np.dtype(dtype)], "ids of this type cannot name every row of the field"
    rng = np.random.default_rng(seed)
    order = rng.permutation(B)
    ids = np.stack([(g - g[0])[(order + c) % len(g)] for c, g in enumerate(groups)], 1).astype(dtype)
    return layout(vocab, world, rpr, offs), ids


# (rows_per_rank, world, n_fields, batch, id type): rpr in {1, 3, a prime near 1e7, 2^31 - 1}, world in {1, 2, 5, 64},
# n_fields in {1, 3, 26}, batch in {1, 255, 256, 257, 1000}; rpr 2^31 - 1 with world 5 / 64 puts offsets above 2^32
BUCKET_CASES = [(1, 1, 1, 1, np.int32), (1, 5, 3, 256, np.float32), (1, 64, 26, 257, np.int32),
                (3, 2, 3, 255, np.int64), (3, 64, 26, 1000, np.float32), (9_999_907, 1, 3, 257, np.int32),
                (9_999_907, 2, 3, 1000, np.float32), (9_999_907, 5, 3, 1000, np.int32),
                (9_999_907, 64, 26, 256, np.int64), (9_999_907, 64, 26, 1000, np.int32),
                (RPR_MAX, 1, 1, 256, np.int32), (RPR_MAX, 2, 1, 1000, np.int64), (RPR_MAX, 5, 3, 255, np.int64),
                (RPR_MAX, 64, 26, 1, np.int64), (RPR_MAX, 64, 26, 257, np.int64), (RPR_MAX, 64, 1, 1000, np.int64)]


def _bid(c):
    return "-".join(np.dtype(x).name if isinstance(x, type) else str(x) for x in c)


def fp64_quotient(row, rpr):
    """shard_owner's first guess: trunc((double)row * (1.0 / rpr)), before the +-1 fix-up."""
    return (np.asarray(row, F64) * (1.0 / F64(rpr))).astype(I64)


# rs_shard_field_route / _row_route: (name, vocab, world, rows_per_rank | None, slot_stride extra, rec_stride extra,
# batch, id type).  "straddle": rpr 115 leaves owner 7 of 8 without a row (n_owned = 0), field 1 lies in four owners,
# field 4 in two.  "grid": 4096 x 8 x 80 words > 8192 x 256 threads, the grid-stride loop's second trip.
ROUTE_CASES = [
    ("world1", [7, 1, 30, 5], 1, None, 0, 0, 17, np.int32),
    ("world3", [11, 3, 40, 1, 9, 25, 2, 60, 8, 5, 33, 4, 17], 3, None, 2, 0, 65, np.int64),
    ("straddle", [50, 330, 20, 100, 150, 50, 60, 40], 8, 115, 0, 8, 33, np.float32),
    ("straddle-wide", [50, 330, 20, 100, 150, 50, 60, 40], 8, 115, 3, 8, 257, np.int32),
    ("grid", [3 + (c * 7) % 11 for c in range(80)], 8, None, None, 0, 4096, np.int32),
]


def route_case(c):
    name, vocab, world, rpr, s_extra, r_extra, B, dtype = c
    L = layout(vocab, world, rpr)
    S = L.F if s_extra is None else L.slot_stride + s_extra
    rng = np.random.default_rng(len(name) + B)
    return L, S, S + r_extra, random_ids(rng, B, L.vocab, dtype)


def owners_of_fields(L):
    return [int(min((L.offs[c] + L.vocab[c] - 1) // L.rpr, L.world - 1) - min(L.offs[c] // L.rpr, L.world - 1)) + 1
            for c in range(L.F)]


# rs_gather_rows / rs_unpermute_rows / rs_scatter_rows: (k, n, table offset, out offset) in floats from a 16-B boundary
GATHER_CASES = [(1, 63, 0, 0), (3, 1000, 0, 0), (4, 64, 0, 0), (8, 65, 0, 0), (16, 1, 0, 0), (16, 1000, 0, 0),
                (20, 63, 0, 0), (64, 65, 0, 0), (16, 64, 1, 0), (16, 65, 0, 1), (8, 1000, 1, 0), (8, 63, 0, 1),
                (4, 1, 0, 0), (1, 1, 0, 0)]


# rs_shard_dedup_route (+ rs_shard_dedup_grad with k): (name, vocab, world, rows_per_rank | None, batch, id type,
# how the ids are drawn, k of the gradient)
def _dedup_ids(how, rng, B, L, dtype):
    if how == "zipf":
        ids = np.minimum(rng.zipf(1.3, size=(B, L.F)) - 1, L.vocab[None, :] - 1)
    elif how == "one":       # one hot row per field
        ids = np.broadcast_to(rng.integers(0, L.vocab)[None, :], (B, L.F))
    elif how == "distinct":  # every lookup of a field another row
        ids = np.stack([rng.permutation(int(v))[:B] for v in L.vocab], 1)
    elif how == "hot700":    # the row of lookup 0 700 times in field 0, the rest spread
        ids = random_ids(rng, B, L.vocab)
        ids[rng.permutation(B - 1)[:699] + 1, 0] = ids[0, 0]
    elif how == "hot1500":
        ids = random_ids(rng, B, L.vocab)
        ids[rng.permutation(B)[:1500], 0] = 5
    elif how == "chunks":    # field 0 grouped: row A 256 lookups (ends at a chunk end), row B 512 (crosses, ends at
        # one)
        ids = random_ids(rng, B, L.vocab)
        rest = rng.permutation(B - 2) + 2
        ids[0, 0], ids[1, 0] = 0, 1
        ids[rest[:255], 0], ids[rest[255:766], 0] = 0, 1
        ids[rest[766:], 0] = 2 + rng.permutation(int(L.vocab[0]) - 2)[:B - 768]
    else:
        ids = random_ids(rng, B, L.vocab)
    return np.ascontiguousarray(ids).astype(dtype)


V26 = [5, 1200, 17, 3000, 2, 90, 640, 33, 7, 2100, 450, 11, 1, 76, 980, 260, 19, 3, 1500, 88, 610, 42, 9, 330, 2750, 14]
DEDUP_CASES = [
    ("lw0-1024", V26[:6], 3, None, 1024, np.int32, "zipf", 4),
    ("lw1-1025", V26[:5], 3, None, 1025, np.int64, "zipf", 16),
    ("lw1-2048", V26[:3], 2, None, 2048, np.float32, "zipf", 1),
    ("lw2-2049", V26[:3], 2, None, 2049, np.int32, "zipf", 4),
    ("lw2-4096", V26[:2], 8, None, 4096, np.int64, "zipf", 16),
    ("sort-4097", [700, 6000], 3, None, 4097, np.float32, "zipf", 4),
    ("sort-f1025", [2 + c % 5 for c in range(1025)], 4, None, 2, np.int32, "rand", 1),
    ("hash-f1024", [2 + c % 5 for c in range(1024)], 4, None, 2, np.int64, "rand", 4),
    ("hash-f257", [2 + c % 5 for c in range(257)], 3, None, 5, np.float32, "rand", 16),
    ("world4096", [8192], 4096, 2, 300, np.int32, "rand", 4),
    ("world4097", [8194], 4097, 2, 300, np.int32, "rand", 4),
    ("one-row", V26[:8], 3, None, 300, np.int32, "one", 16),
    ("distinct", [5000, 7000, 4100], 5, None, 1500, np.int64, "distinct", 4),
    ("hot700", [4000, 30], 2, None, 1100, np.int32, "hot700", 65),
    ("hot700-k16", [4000, 30], 2, None, 1100, np.int32, "hot700", 16),
    ("hot1500", [9000, 50], 3, None, 4097, np.int32, "hot1500", 65),
    ("hot1500-k4", [9000, 50], 3, None, 4097, np.int64, "hot1500", 4),
    ("chunks", [3000, 8], 2, None, 1100, np.int32, "chunks", 16),
    ("chunks-k1", [3000, 8], 2, None, 1100, np.float32, "chunks", 1),
    ("tiny", V26[:4], 2, None, 40, np.int64, "zipf", 16),  # n <= seg_chunk: no dedup_grad_cross launch
]


def dedup_case(c):
    name, vocab, world, rpr, B, dtype, how, k = c
    L = layout(vocab, world, rpr)
    rng = np.random.default_rng(sum(map(ord, name)))
    return L, _dedup_ids(how, rng, B, L, dtype), k, rng


def fm_params(rng, nd, F, k, kfm):
    d = nd + F * k
    return SimpleNamespace(nd=nd, F=F, k=k, kfm=kfm, d=d, w0=np.asarray([0.1], F32),
                           w1=(_nrm(rng, d) / np.sqrt(d)).astype(F32), v=(_nrm(rng, d, kfm) / np.sqrt(d)).astype(F32))


# rs_shard_owner_fm (and, at k <= 16, rs_shard_owner_fm_grad): (name, n_owned, field_lo, n_fields, kfm, k, nd, n_pairs,
# rec_stride - n_owned, partial_stride - P): n_owned in {0, 1, 4, 5, 8, 9, 32, 33}, kfm in {1, 10, 15, 16, 31}, k in
# {4, 8, 16, 32, 64}, nd in {0, 1, 5, 13}, n_pairs in {1, 15, 16, 17, 49}: a covering selection
OWNER_CASES = [
    ("own0", 0, 3, 40, 10, 16, 13, 17, 2, 3), ("own1", 1, 39, 40, 1, 4, 0, 1, 1, 0),
    ("own4", 4, 2, 40, 15, 8, 1, 15, 3, 3), ("own5", 5, 7, 40, 10, 16, 5, 16, 1, 0),
    ("own8", 8, 1, 40, 31, 32, 13, 17, 2, 3), ("own9", 9, 30, 40, 10, 64, 0, 49, 1, 0),
    ("own32", 32, 8, 40, 15, 16, 5, 16, 4, 3), ("own33", 33, 7, 40, 10, 8, 13, 49, 1, 0),
    ("own33-nt2", 33, 5, 40, 16, 4, 1, 15, 2, 3), ("own32-nt2", 32, 0, 40, 31, 16, 0, 17, 1, 0),
    ("own9-nt2", 9, 4, 40, 16, 8, 5, 49, 1, 3), ("const26", 26, 3, 40, 10, 16, 13, 49, 2, 0),
    ("const26-nd0", 26, 0, 26, 10, 16, 0, 17, 1, 3),
]
SHARD_ROWS = 37


def owner_case(c, bad=False):
    name, n_owned, lo, F, kfm, k, nd, n_pairs, rec_x, pst_x = c
    rng = np.random.default_rng(sum(map(ord, name)))
    m = fm_params(rng, nd, F, k, kfm)
    shard = (_nrm(rng, SHARD_ROWS, k) * 0.5).astype(F32)
    recv = np.full((n_pairs, n_owned + rec_x), 0x7ffffff0, I32)  # the words past n_owned are never read
    rows = rng.integers(0, SHARD_ROWS, (n_pairs, n_owned))
    recv[:, :n_owned] = np.where(rng.random(rows.shape) < 0.2, -1, rows)
    if bad and n_owned:
        recv[n_pairs // 2, n_owned // 2] = SHARD_ROWS  # one past the shard: the flag
    gs = np.concatenate([_nrm(rng, n_pairs, kfm) * 0.5, _nrm(rng, n_pairs, 1) * 0.1], 1).astype(F32)
    return SimpleNamespace(m=m, shard=shard, recv=recv, lo=lo, n_owned=n_owned, n_pairs=n_pairs,
                           P=partial_width(kfm), pst=partial_width(kfm) + pst_x, gs=gs)


# rs_shard_fm_combine / _combine_grad: (world, kfm, nd, batch, gs_stride - (kfm + 1), loss): world in {1, 3, 64}, kfm in
# {1, 14, 15, 16, 30, 31}, nd in {0, 1, 13}, batch in {1, 15, 16, 17, 257}
COMBINE_CASES = [(1, 1, 0, 1, 0, True), (3, 14, 1, 15, 3, False), (64, 15, 13, 16, 0, True), (1, 16, 13, 17, 3, True),
                 (3, 30, 0, 257, 0, False), (64, 31, 1, 17, 3, True), (3, 15, 0, 257, 3, True),
                 (1, 31, 13, 16, 0, False),
                 (64, 14, 13, 1, 0, True), (3, 16, 1, 257, 3, False)]


def combine_case(c):
    world, kfm, nd, B, gs_x, loss = c
    rng = np.random.default_rng(world * 1000 + kfm * 10 + nd)
    m = fm_params(rng, nd, 4, 8, kfm)
    P = partial_width(kfm)
    part = np.zeros((world, B, P), F32)
    part[:, :, :kfm + 1] = _nrm(rng, world, B, kfm + 1) * 0.5 / np.sqrt(world)
    part[:, :, kfm + 1] = np.abs(_nrm(rng, world, B)) * 0.5 / world
    return SimpleNamespace(m=m, part=part, dense=rng.random((B, nd)).astype(F32), B=B, world=world, P=P,
                           labels=(rng.random(B) < 0.4).astype(F32), scale=1.0 / (B * world), gst=kfm + 1 + gs_x,
                           loss=loss)


# rs_rows_fm_fwd: (k, nd, batch), 5 fields, kfm 10: k in {3, 16}, nd in {0, 13}, batch in {1, 17}
ROWS_FM_CASES = [(3, 0, 1), (3, 13, 17), (16, 0, 17), (16, 13, 1)]


def rows_fm_case(c):
    k, nd, B = c
    rng = np.random.default_rng(k * 100 + nd + B)
    m = fm_params(rng, nd, 5, k, 10)
    return m, (_nrm(rng, B, 5 * k) * 0.5).astype(F32), rng.random((B, nd)).astype(F32)


# --------------------------------------------------------------------------
# A. CPU: the references are pinned
# --------------------------------------------------------------------------
def _sh(L, rank=0, **kw):
    """The attributes CpuOps reads from a ShardedEmbeddingFM."""
    return SimpleNamespace(offsets=torch.as_tensor(L.offs), rows_per_rank=L.rpr, world=L.world, rank=rank,
                           owner_field_ranges=[tuple(int(x) for x in r) for r in L.owner_fields],
                           slot_stride=L.slot_stride, **kw)


def test_integer_references_equal_cpuops():
    """Valid ids: ref_bucketize, ref_slot_bucketize, ref_field_route (send and slot_of) and ref_dedup_route in row
    order equal the test double of tests/test_sharded_gloo.py word for word."""
    cpu = CpuOps()
    rng = np.random.default_rng(3)
    L = layout(V26, 3)
    ids = random_ids(rng, 70, L.vocab, I32, hot=0.5)
    t = torch.as_tensor(ids)
    counts, perm, send = ref_bucketize(ids, L)
    for mine, theirs in zip((counts, perm, send), cpu.bucketize(t, torch.as_tensor(L.offs), None, L.rpr, L.world)):
        np.testing.assert_array_equal(mine, theirs.numpy())
    for cap in (int(counts.max()), int(counts.max()) - 1):
        cpu.overflow = False
        slot_t, send_t = cpu.slot_bucketize(t, torch.as_tensor(L.offs), None, L.rpr, L.world, cap)
        _, slot, send, over = ref_slot_bucketize(ids, L, cap)
        np.testing.assert_array_equal(slot, slot_t.numpy())
        np.testing.assert_array_equal(send, send_t.numpy())
        assert over == cpu.overflow and over == (cap < counts.max())
    sh = _sh(L)
    S = L.slot_stride
    send_t, slot_t = torch.empty(L.world * 70 * S, dtype=torch.int32), torch.empty(70, L.F, dtype=torch.int32)
    cpu.row_route(sh, t, send_t, slot_t)
    out, slot = ref_field_route(ids, L, S)
    np.testing.assert_array_equal(out.reshape(-1), send_t.numpy())
    np.testing.assert_array_equal(slot, slot_t.numpy())
    np.testing.assert_array_equal(out.reshape(-1), cpu.field_route(sh, t, torch.empty_like(send_t)).numpy())
    distinct = max(np.unique(rows_of(ids, L)[1][rows_of(ids, L)[2] == o]).size for o in range(L.world))
    for cap in (distinct, distinct - 1):
        rb = {"cap": cap, "send": torch.empty(L.world * cap, dtype=torch.int32),
              "slot_of": torch.empty(70, L.F, dtype=torch.int32)}
        cpu.dedup_overflow = False
        cpu.dedup_route(sh, t, rb)
        send, slot, over = ref_dedup_route(ids, L, cap, "row")
        np.testing.assert_array_equal(send, rb["send"].numpy())
        np.testing.assert_array_equal(slot, rb["slot_of"].numpy().reshape(-1))
        assert over == cpu.dedup_overflow and over == (cap < distinct)
        for order in ("row", "first"):
            s2, sl2, ov2 = ref_dedup_route(ids, L, cap, order)
            assert check_dedup_route(ids, L, cap, s2, sl2) == ov2 == over


def test_float_references_equal_cpuops():
    """ref_owner_fm, ref_combine and ref_bce equal CpuOps' float64 partial protocol within 1e-12."""
    cpu = CpuOps()
    rng = np.random.default_rng(5)
    nd, k, kfm, B = 5, 4, 6, 9
    L = layout([7, 30, 12, 9, 20], 2)
    m = fm_params(rng, nd, L.F, k, kfm)
    P = partial_width(kfm)
    ids = random_ids(rng, B, L.vocab, I32)
    out, _ = ref_field_route(ids, L, L.slot_stride)
    table = (_nrm(rng, L.world * L.rpr, k) * 0.5).astype(F32)
    parts, parts64 = np.zeros((L.world, B, P), F32), np.zeros((L.world, B, P))
    for o in range(L.world):
        sh = _sh(L, o, table_shard=torch.as_tensor(table[o * L.rpr:(o + 1) * L.rpr]), v=torch.as_tensor(m.v),
                 w1=torch.as_tensor(m.w1.reshape(-1, 1)), w0=torch.as_tensor(m.w0), nd=nd, k=k, kfm=kfm,
                 partial_width=P)
        theirs = cpu.owner_partials(sh, torch.as_tensor(out[o].astype(I32)), B, torch.zeros(B * P)).numpy()
        lo, n = L.owner_fields[o]
        mine, flag = ref_owner_fm(out[o], lo, n, table[o * L.rpr:(o + 1) * L.rpr], L.rpr, nd, k, m.w1, m.v, kfm)
        assert flag == 0
        # CpuOps rounds its float64 result to the float32 buffer: compare what was rounded
        np.testing.assert_allclose(mine.astype(F32), theirs.reshape(B, P)[:, :kfm + 2], rtol=0, atol=0)
        parts[o, :, :kfm + 2], parts64[o, :, :kfm + 2] = mine, mine
    dense = rng.random((B, nd)).astype(F32)
    labels = (rng.random(B) < 0.5).astype(F32)
    z, S = ref_combine(parts, dense, nd, m.w0, m.w1, m.v, kfm)
    g, loss = ref_bce(z, labels, 0.25)
    # the double's own formula, in float64, on the same float32 inputs: 1e-12; then the double itself, whose
    # float64 results are rounded to its float32 buffers: equal after the same rounding
    p = parts.astype(F64).sum(0)
    d, v, w1 = dense.astype(F64), m.v.astype(F64), m.w1.astype(F64)
    S2 = p[:, :kfm] + d @ v[:nd]
    z2 = p[:, kfm] + d @ w1[:nd] + float(m.w0[0]) + 0.5 * ((S2 ** 2).sum(1) - p[:, kfm + 1] -
                                                            (d * d) @ (v[:nd] ** 2).sum(1))
    np.testing.assert_allclose(z, z2, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(S, S2, rtol=1e-12, atol=1e-12)
    sh = _sh(L, 0, v=torch.as_tensor(m.v), w1=torch.as_tensor(m.w1.reshape(-1, 1)), w0=torch.as_tensor(m.w0), nd=nd,
             k=k, kfm=kfm, partial_width=P)
    lt, gt, st = torch.zeros(B, 1), torch.zeros(B, kfm + 1), torch.zeros(B)
    cpu.combine_grad(sh, torch.as_tensor(parts), torch.as_tensor(dense), torch.as_tensor(labels), 0.25, lt, gt, st)
    np.testing.assert_array_equal(z.astype(F32), lt.numpy()[:, 0])
    np.testing.assert_array_equal(S.astype(F32), gt.numpy()[:, :kfm])
    np.testing.assert_array_equal(g.astype(F32), gt.numpy()[:, kfm])
    np.testing.assert_array_equal(loss.astype(F32), st.numpy())
    out_t = torch.zeros(B, 1)
    cpu.combine(sh, torch.as_tensor(parts), torch.as_tensor(dense), out_t)
    np.testing.assert_array_equal(z.astype(F32), out_t.numpy()[:, 0])
    # ... and the sharded FM equals the plain FM on the gathered x
    ok, row, _, _ = rows_of(ids, L)
    x = np.concatenate([dense, table[row].reshape(B, -1)], 1)
    np.testing.assert_allclose(ref_combine(parts64, dense, nd, m.w0, m.w1, m.v, kfm)[0], ref_fm(x, m.w0, m.w1, m.v),
                               rtol=1e-12, atol=1e-12)


def test_dedup_grad_and_scatter_equal_add_at():
    rng = np.random.default_rng(7)
    slot = rng.integers(-1, 6, 40)
    g = _nrm(rng, 40, 3)
    acc = np.zeros((8, 3))
    np.add.at(acc, slot[slot >= 0], g[slot >= 0].astype(F64))
    dst, written = ref_dedup_grad(g, slot, 8)
    np.testing.assert_array_equal(dst, acc)
    np.testing.assert_array_equal(written, np.isin(np.arange(8), slot))
    # the slot scatter: one lookup per slot, so add.at onto zeros is the assignment
    slot = np.where(rng.random(40) < 0.3, -1, rng.permutation(64)[:40])
    src = _nrm(rng, 8, 5 * 3 + 5)
    acc = np.zeros((64, 3), F32)
    np.add.at(acc, slot[slot >= 0], src[:, :15].reshape(-1, 3)[slot >= 0])
    got = ref_scatter(src, slot, 3, np.zeros((64, 3), F32))
    np.testing.assert_array_equal(got, acc)


def test_float32_ids_decode_as_the_library():
    ids = np.asarray([[-1.0, -0.5, 0.0, 2.9, 3.0, np.nan, np.inf, -np.inf, 2.9999998]], F32)
    ok, idv = decode(ids, [3] * 9)
    assert ok.tolist() == [[False, True, True, True, False, False, False, False, True]]
    assert idv.tolist() == [[0, 0, 0, 2, 0, 0, 0, 0, 2]]
    for dt in (I32, I64):
        ok, idv = decode(np.asarray([[-1, 0, 2, 3]], dt), [3] * 4)
        assert ok.tolist() == [[False, True, True, False]] and idv.tolist() == [[0, 0, 2, 0]]


# --------------------------------------------------------------------------
# A. CPU: the cases are what they claim, and every branch has one
# --------------------------------------------------------------------------
def test_boundary_cases_reach_every_owner_boundary_and_both_fixups():
    """Every (rows_per_rank, world) of BUCKET_CASES asks, in some case, for the rows o * rpr - 1, o * rpr and
    o * rpr + 1 of every owner; the named parameter values all occur; rows above 2^32 occur; and the fp64 quotient
    of shard_owner is one too small somewhere in the list, so the ++o arm of the fix-up decides a result.  (That
    takes 1 / rpr rounded down by more than a quarter ulp and an owner o whose o * rpr sits just above a power of
    two times rpr: of the primes within 100 of 1e7 only 9,999,907 has it, at o = 1, 2, 4, 7, 8, 14, ..; rpr 3 and
    2^31 - 1 never do.  The --o arm would need o * ulp >= 1 / rpr: no row below 2^52 reaches it, so no case can.)"""
    seen, need_inc, need_dec, big = {}, 0, 0, False
    for c in BUCKET_CASES:
        rpr, world, F, B, dtype = c
        L, ids = boundary_case(*c)
        assert np.all(L.offs[1:] >= (L.offs + L.vocab)[:-1]), "fields overlap"
        ok, row, owner, local = rows_of(ids, L)
        assert ok.all() and local.max() < rpr and owner.max() < world
        seen.setdefault((rpr, world), set()).update(row.tolist())
        q = fp64_quotient(row, rpr)
        assert np.all(np.abs(q - row // rpr) <= 1)
        need_inc += int(np.sum(q < row // rpr))
        need_dec += int(np.sum(q > row // rpr))
        big |= bool(row.max() > 1 << 32) and bool(L.offs.max() > 1 << 32)
    for (rpr, world), rows in seen.items():
        want = {r for o in range(world + 1) for r in (o * rpr - 1, o * rpr, o * rpr + 1) if 0 <= r < world * rpr}
        assert want <= rows, (rpr, world, sorted(want - rows)[:5])
    assert {c[0] for c in BUCKET_CASES} == {1, 3, 9_999_907, RPR_MAX} and {c[1] for c in BUCKET_CASES} == {1, 2, 5, 64}
    assert {c[2] for c in BUCKET_CASES} == {1, 3, 26} and {c[3] for c in BUCKET_CASES} == {1, 255, 256, 257, 1000}
    assert {np.dtype(c[4]) for c in BUCKET_CASES} == {np.dtype(t) for t in DTYPES}
    assert big and need_inc > 0 and need_dec == 0, (need_inc, need_dec)


def test_route_cases_straddle_as_named():
    L = layout(*ROUTE_CASES[2][1:4])
    per_field = owners_of_fields(L)
    assert 2 in per_field and 4 in per_field and max(per_field) == 4, per_field
    assert (L.owner_fields[:, 1] == 0).any(), "an owner without a field"
    for c in ROUTE_CASES:
        L, S, R, ids = route_case(c)
        assert S >= L.slot_stride and S <= L.F and R >= S
    L, S, R, ids = route_case(ROUTE_CASES[-1])
    assert L.world * ids.shape[0] * S > 8192 * 256, "the grid-stride loop's second trip"
    assert {c[2] for c in ROUTE_CASES} == {1, 3, 8}
    assert any(c[4] for c in ROUTE_CASES) and any(c[5] for c in ROUTE_CASES)


def _launch_conditions(func):
    """The launcher's own if / else-if conditions in front of each kernel<<<...>>> of `func` in shard.hip, as
    Python expressions over k, n, and the pointers' offsets."""
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "recommender_system_amd",
                            "csrc", "shard.hip")).read()
    body = src[src.index(f'extern "C" int {func}('):]
    body = body[:body.index("\n}\n")]
    out = []
    for cond, kern in re.findall(r"(?:if \((.*)\)|else)\n\s+(\w+(?:<\d>)?)<<<", body):
        py = cond.replace("&&", "and").replace("(uintptr_t)", "").replace("(1 << 29)", str(1 << 29)) or "True"
        out.append((py, kern))
    return out


def test_row_kernels_dispatch_is_the_launchers():
    """gather_branch / unpermute_branch equal the launchers' own conditions, evaluated from the source, on every
    (k, n, pointer offset): a float4 kernel is never chosen for a pointer that is not 16-B aligned (a launcher
    that dropped the alignment test fails here, without a misaligned float4 access ever being run)."""
    g, u = _launch_conditions("rs_gather_rows"), _launch_conditions("rs_unpermute_rows")
    assert [k for _, k in g] == ["gather_rows_k16", "gather_rows_kernel<4>", "gather_rows_kernel<1>"]
    assert [k for _, k in u] == ["unpermute_rows_kernel<4>", "unpermute_rows_kernel<1>"]
    for k in (1, 3, 4, 8, 12, 16, 20, 64):
        for n in (1, 1000, 1 << 29):
            for a in (0, 4, 8, 16):
                for b in (0, 4, 12):
                    env = dict(k=k, n=n, table=0x7000 + a, out=0x9000 + b, src=0x7000 + a, dst=0x9000 + b)
                    assert next(kn for c, kn in g if eval(c, {}, env)) == gather_branch(k, n, a, b), (k, n, a, b)
                    assert next(kn for c, kn in u if eval(c, {}, env)) == unpermute_branch(k, a, b), (k, a, b)
                    if a % 16 or b % 16:
                        assert gather_branch(k, n, a, b).endswith("<1>") and unpermute_branch(k, a, b).endswith("<1>")


def test_every_branch_is_named_by_a_case():
    # rs_shard_dedup_route: LW 0 / 1 / 2 on both sides of 1024 and 2048, the chunk of dedup_scatter_f 1, 2 and 4, the
    # sort path by batch, by n_fields and by world
    routes = {c[0]: dedup_route_branch(c[4], len(c[1]), c[2]) for c in DEDUP_CASES}
    assert {"hash LW=0 chunk=1", "hash LW=1 chunk=1", "hash LW=2 chunk=1", "hash LW=0 chunk=2", "hash LW=0 chunk=4",
            "sort"} == set(routes.values()), routes
    assert routes["lw0-1024"][:9] == "hash LW=0" and routes["lw1-1025"][:9] == "hash LW=1" and \
        routes["lw1-2048"][:9] == "hash LW=1" and routes["lw2-2049"][:9] == "hash LW=2" and \
        routes["lw2-4096"][:9] == "hash LW=2"
    assert [routes[n] for n in ("sort-4097", "sort-f1025", "world4097")] == ["sort"] * 3
    assert routes["hash-f1024"] == "hash LW=0 chunk=4" and routes["world4096"] == "hash LW=0 chunk=1"
    assert dh_per_field(4096, 1024, 4096) and not (dh_per_field(4097, 1, 1) or dh_per_field(1, 1025, 1) or
                                                   dh_per_field(1, 1, 4097))
    # rs_shard_dedup_grad: the three grouping kernels and the sorted order, seg_chunk 256 and 512, one piece and more
    grads = {c[0]: dedup_grad_branch(c[4], len(c[1]), c[2], c[7]) for c in DEDUP_CASES}
    for want in ("dedup_group_f<0>", "dedup_group_f<1>", "dedup_group_f<2>", "sorted", "C=256", "C=512", "piece+cross"):
        assert any(want in g for g in grads.values()), want
    assert any(g.endswith(" piece") for g in grads.values())
    assert [seg_chunk(k) for k in (1, 4, 16, 64, 65, 128, 129)] == [256, 256, 256, 256, 512, 512, 1024]
    assert grads["hot700"] == "dedup_group_f<1> C=512 piece+cross" and grads["hot1500"] == "sorted C=512 piece+cross"
    assert {c[7] for c in DEDUP_CASES} == {1, 4, 16, 65}
    # the row kernels
    assert {gather_branch(k, n, 4 * a, 4 * b) for k, n, a, b in GATHER_CASES} == \
        {"gather_rows_k16", "gather_rows_kernel<4>", "gather_rows_kernel<1>"}
    assert {unpermute_branch(k, 4 * a, 4 * b) for k, n, a, b in GATHER_CASES} == \
        {"unpermute_rows_kernel<4>", "unpermute_rows_kernel<1>"}
    for k in (16, 8):  # the scalar kernel by the table's alignment alone and by the output's alone
        assert {(a, b) for kk, n, a, b in GATHER_CASES if kk == k} >= {(0, 0), (1, 0), (0, 1)}
    assert {c[0] for c in GATHER_CASES} == {1, 3, 4, 8, 16, 20, 64} and {c[1] for c in GATHER_CASES} == \
        {1, 63, 64, 65, 1000}
    # launch_pipe_kv's six lines and launch_pipe4's constant shape, by the owner part; the combine takes two of them
    lines = {}
    for c in OWNER_CASES:
        name, n_owned, lo, F, kfm, k, nd = c[:7]
        if n_owned:
            lines.setdefault(pipe_line(pipe_branch(nd, F, k, kfm, n_owned)), []).append(name)
    assert set(lines) == PIPE_LINES, set(lines) ^ PIPE_LINES
    assert pipe_branch(13, 40, 16, 10, 26) == "shard_fm_pipe<4,1,16,1,26,10>" == pipe_branch(0, 26, 16, 10, 26)
    assert pipe_branch(0, 40, 16, 10, 25) == "shard_fm_pipe<4,1,16,1>" == pipe_branch(0, 40, 16, 11, 26)
    assert {pipe_line(pipe_branch(c[2], 4, 8, c[1], 0)) for c in COMBINE_CASES} == {"1,4,1", "2,16,1"}
    assert {c[1] for c in OWNER_CASES} == {0, 1, 4, 5, 8, 9, 26, 32, 33} and {c[4] for c in OWNER_CASES} == \
        {1, 10, 15, 16, 31} and {c[5] for c in OWNER_CASES} == {4, 8, 16, 32, 64} and \
        {c[6] for c in OWNER_CASES} == {0, 1, 5, 13} and {c[7] for c in OWNER_CASES} == {1, 15, 16, 17, 49}
    assert {c[0] for c in COMBINE_CASES} == {1, 3, 64} and \
        {c[1] for c in COMBINE_CASES} == {1, 14, 15, 16, 30, 31} and \
        {c[2] for c in COMBINE_CASES} == {0, 1, 13} and {c[3] for c in COMBINE_CASES} == {1, 15, 16, 17, 257}
    # fm_geom and the partial width, against the library's host query
    lib = _lib.lib()
    for kfm in range(0, 40):
        assert lib.rs_fm_partial_width(kfm) == partial_width(kfm)
    assert [fm_geom(0, 4, k, 10)["KV"] for k in (4, 8, 16, 32, 64)] == [1, 2, 4, 8, 16]
    assert [fm_geom(0, 4, 8, kfm)["NT"] for kfm in (1, 14, 15, 16, 30, 31)] == [1, 1, 1, 2, 2, 2]
    assert not fm_geom(0, 4, 12, 10)["mfma"] and not fm_geom(0, 4, 8, 32)["mfma"]


def test_dedup_cases_hold_the_segments_they_name():
    """The hot rows are as long as named, "chunks" has a segment that ends exactly at a chunk end and one that
    crosses into a chunk it fills, and a 700-lookup row covers a whole chunk between its first and last piece."""
    L, ids, k, _ = dedup_case(next(c for c in DEDUP_CASES if c[0] == "hot700"))
    assert np.sum(ids[:, 0] == ids[0, 0]) == 700 and 700 > 2 * 256
    L, ids, k, _ = dedup_case(next(c for c in DEDUP_CASES if c[0] == "hot1500"))
    assert np.sum(ids[:, 0] == 5) >= 1500
    L, ids, k, _ = dedup_case(next(c for c in DEDUP_CASES if c[0] == "chunks"))
    assert ids[0, 0] == 0 and ids[1, 0] == 1 and np.sum(ids[:, 0] == 0) == 256 and np.sum(ids[:, 0] == 1) == 512
    assert seg_chunk(k) == 256  # field 0 grouped in order of first occurrence: [0, 256) row 0, [256, 768) row 1
    L, ids, k, _ = dedup_case(next(c for c in DEDUP_CASES if c[0] == "distinct"))
    assert all(np.unique(ids[:, c]).size == ids.shape[0] for c in range(L.F))
    L, ids, k, _ = dedup_case(next(c for c in DEDUP_CASES if c[0] == "world4096"))
    assert owners_of_fields(L) == [4096] and L.world * L.rpr == 8192


# --------------------------------------------------------------------------
# A. CPU: every bound of every RS_REQUIRE, both sides, without a launch.  The accepted side of a bound is shown by a
# LATER check refusing the call (an id_kind of 3, a partial_stride below P, kfm 32): nothing is launched on dummy
# pointers.  Where no later check exists (the last one of an entry) the accepted side is a GPU case below.
# --------------------------------------------------------------------------
def _unsupported(status, *words):
    msg = _lib.lib().rs_last_error_string()
    assert status == -3, (status, msg)
    for w in words:
        assert w in msg, msg


def test_argument_checks_both_sides_without_device():
    lib = _lib.lib()
    p = [_p(i) for i in range(1, 12)]
    assert lib.rs_shard_workspace_size(1000, 64) > 0 and lib.rs_shard_workspace_size(1000, 65) == -1
    assert lib.rs_shard_workspace_size(1000, 0) == -1 and lib.rs_shard_workspace_size(-1, 4) == -1
    assert lib.rs_shard_dedup_workspace_size(1000, 4097) > 0 and lib.rs_shard_dedup_workspace_size(1000, 0) == -1
    B31 = 1 << 31

    def bucket(world=4, rpr=10, kind=3, F=3, batch=5):
        return lib.rs_shard_bucketize(p[0], kind, F, p[1], p[2], F, batch, rpr, world, p[3], p[4], p[5], p[6], None,
                                      None)

    def slot(world=4, rpr=10, kind=3, F=3, batch=5, cap=7):
        return lib.rs_shard_slot_bucketize(p[0], kind, F, p[1], p[2], F, batch, rpr, world, cap, p[3], p[4], p[5],
                                           p[6], None, p[7], None)

    def froute(world=4, rpr=10, kind=3, F=3, batch=5, S=2, R=2):
        return lib.rs_shard_field_route(p[0], kind, F, p[1], p[2], F, batch, rpr, world, p[3], S, R, p[4], None, None)

    def rroute(world=4, rpr=10, kind=3, F=3, batch=5, S=2):
        return lib.rs_shard_row_route(p[0], kind, F, p[1], p[2], F, batch, rpr, world, p[3], S, p[4], p[5], None, None)

    def dedup(world=4, rpr=10, kind=3, F=3, batch=5, cap=7):
        return lib.rs_shard_dedup_route(p[0], kind, F, p[1], p[2], F, batch, rpr, world, cap, p[3], p[4], p[5], None,
                                        None, None)

    for f, name in ((bucket, b"rs_shard_bucketize"), (slot, b"rs_shard_slot_bucketize"),
                    (froute, b"rs_shard_field_route"), (rroute, b"rs_shard_row_route")):
        _refused(f(), name, b"bad id_kind")          # every other argument accepted: the id kind alone refuses
        _refused(f(kind=-1), name, b"bad id_kind")
        _refused(f(world=64), name, b"bad id_kind")  # world 64 passes the shape check ...
        _refused(f(world=65), name, b"bad shape")    # ... 65 does not
        _refused(f(world=0), name, b"bad shape")
        _refused(f(rpr=B31 - 1), name, b"bad id_kind")
        _refused(f(rpr=B31), name, b"must fit int32")
        _refused(f(rpr=0), name, b"bad shape")
    _refused(slot(cap=1), b"bad id_kind")
    _refused(slot(cap=0), b"cap >= 1")
    for f in (froute, rroute):
        _refused(f(S=1, R=1) if f is froute else f(S=1), b"bad id_kind")
        _refused(f(S=3, R=3) if f is froute else f(S=3), b"bad id_kind")   # slot_stride = n_fields
        _refused(f(S=0, R=2) if f is froute else f(S=0), b"slot_stride")
        _refused(f(S=4, R=4) if f is froute else f(S=4), b"slot_stride")   # n_fields + 1
    _refused(froute(S=2, R=2), b"bad id_kind")
    _refused(froute(S=2, R=1), b"bad shape")                               # rec_stride < slot_stride
    # the dedup route: rows must fit uint32 with 0xffffffff kept for a bad id
    _refused(dedup(), b"rs_shard_dedup_route", b"bad id_kind")
    _refused(dedup(world=2, rpr=0x7fffffff), b"bad id_kind")               # world * rpr = 0xfffffffe
    _refused(dedup(world=1, rpr=0xfffffffe), b"bad id_kind")
    _refused(dedup(world=1, rpr=0xffffffff), b"rows must fit uint32")
    _refused(dedup(world=3, rpr=0x55555555), b"rows must fit uint32")      # = 0xffffffff
    _refused(dedup(world=4097), b"bad id_kind")                            # no bound on world: the sort path
    _refused(dedup(cap=1), b"bad id_kind")
    _refused(dedup(cap=0), b"bad shape")
    _refused(lib.rs_shard_dedup_grad(p[0], 3 * 4 - 1, 3, 4, 5, 2, p[1], p[2], p[3], None), b"rs_shard_dedup_grad")
    _refused(lib.rs_scatter_rows(p[0], 3 * 4 - 1, 3, 4, p[1], 5, p[2], None), b"rs_scatter_rows")
    _refused(lib.rs_gather_rows(p[0], 10, 0, p[1], 5, p[2], None, None), b"rs_gather_rows", b"bad shape")

    # the FM entries: shape -> pointers -> alignment -> the packed image's geometry -> partial_stride
    def owner(kfm=10, k=16, shard=p[1], pst=11, n_owned=2, rec=2, lo=1, F=3):
        return lib.rs_shard_owner_fm(p[0], rec, lo, n_owned, shard, 9, 13, F, k, p[2], kfm, p[3], pst, 5, None, None)

    def combine(kfm=10, k=16, pst=11, world=3):
        return lib.rs_shard_fm_combine(p[0], pst, world, 5, p[1], 13, 13, 3, k, p[2], p[3], kfm, p[4], None)

    def cgrad(kfm=10, k=16, pst=11, gst=None):
        gst = kfm + 1 if gst is None else gst
        return lib.rs_shard_fm_combine_grad(p[0], pst, 3, 5, p[1], 13, 13, 3, k, p[2], p[3], kfm, p[4], 0.5, p[5],
                                            p[6], gst, None, None)

    for f, name in ((owner, b"rs_shard_owner_fm"), (combine, b"rs_shard_fm_combine"),
                    (cgrad, b"rs_shard_fm_combine_grad")):
        _refused(f(), name, b"partial_stride <")               # P(10) = 12: 11 refused, everything before accepted
        _refused(f(kfm=31, pst=35), name, b"partial_stride <")  # kfm 31 has an image (P = 36) ...
        _unsupported(f(kfm=32, pst=64), name)                  # ... 32 has none
        _unsupported(f(k=12), name)
        for k in (4, 8, 16, 32, 64):
            _refused(f(k=k), name, b"partial_stride <")
    _refused(owner(shard=C.c_void_p(0x2004)), b"16-B aligned")
    _refused(owner(shard=C.c_void_p(0x2010)), b"partial_stride <")
    _refused(owner(n_owned=3, rec=2), b"bad shape")            # n_owned > rec_stride
    _refused(owner(n_owned=2, lo=2), b"bad shape")             # field_lo + n_owned > n_fields
    _refused(cgrad(gst=10), b"rs_shard_fm_combine_grad", b"bad shape")  # gs_stride < kfm + 1 (11 accepted above)
    _refused(lib.rs_shard_owner_fm_grad(p[0], 2, 0, 2, p[1], 9, 13, 16, p[2], p[3], 10, p[4], 10, 5, p[5], p[6], p[7],
                                        p[8], None), b"rs_shard_owner_fm_grad", b"bad shape")   # gs_stride 10 < 11
    _refused(lib.rs_shard_owner_fm_grad(p[0], 1, 0, 2, p[1], 9, 13, 16, p[2], p[3], 10, p[4], 11, 5, p[5], p[6], p[7],
                                        p[8], None), b"rs_shard_owner_fm_grad", b"bad shape")   # rec_stride < n_owned
    _refused(lib.rs_shard_owner_fm_grad(p[0], 2, 0, 2, p[1], 9, 13, 16, p[2], p[3], 33, p[4], 34, 5, p[5], p[6], p[7],
                                        p[8], None), b"rs_shard_owner_fm_grad", b"kfm <= 32")

    # the pipelined step: the id kind is checked before the geometry, so kfm 32 shows what the earlier checks accept
    def pipe(world=4, kind=0, kfm=32, shard=p[1], S=2, rpr=10, n_owned=2):
        return lib.rs_shard_fm_pipe(p[0], 0, n_owned, shard, 9, p[2], 13, p[3], p[4], kind, 3, p[5], p[6], rpr, p[7],
                                    S, p[8], world, 5, 13, 3, 16, p[9], p[10], kfm, None, None)

    _unsupported(pipe(), b"rs_shard_fm_pipe")
    _unsupported(pipe(world=64), b"rs_shard_fm_pipe")
    _refused(pipe(world=65), b"rs_shard_fm_pipe", b"bad shape")
    _refused(pipe(kind=3), b"bad id_kind")
    _refused(pipe(shard=C.c_void_p(0x2004)), b"16-B aligned")
    _refused(pipe(S=0), b"bad shape")
    _refused(pipe(S=4), b"bad shape")
    _refused(pipe(S=1, n_owned=2), b"bad shape")
    _unsupported(pipe(rpr=B31 - 1), b"rs_shard_fm_pipe")
    _refused(pipe(rpr=B31), b"must fit int32")
    _refused(lib.rs_rows_fm_fwd(C.c_void_p(0x2004), p[1], 13, 13, 3, 16, p[2], p[3], 10, p[4], 5, None),
             b"rs_rows_fm_fwd", b"16-B aligned")


# --------------------------------------------------------------------------
# A. CPU: conditioning.  What the GPU tests assert, asserted of the same restatement in float32 numpy at a quarter of
# the tolerance: a case that fails here is a bad case (its inputs change, not the bound).
# --------------------------------------------------------------------------
def _sum_ok(got, ref, absum, what, factor=SUM_TOL, extra=0.0):
    """|got - ref| <= factor * sum |terms| (+ extra)."""
    got, ref, absum = _d(got).reshape(np.shape(ref)), _d(ref), _d(absum).reshape(np.shape(ref))
    err = np.abs(got - ref)
    bad = ~(err <= factor * absum + extra + 1e-30)
    assert not bad.any(), (f"{what}: {int(bad.sum())}/{bad.size} outside {factor:g} * sum|terms|; worst "
                           f"{float(np.nanmax(err / (absum + 1e-300))):.3e}")


def dedup_grad_inputs(c):
    """The gradient rows of a dedup case and the slots of a roomy route (cap = the largest distinct count)."""
    L, ids, k, rng = dedup_case(c)
    order = "first" if dh_per_field(ids.shape[0], L.F, L.world) else "row"
    ok, row, owner, _ = rows_of(ids, L)
    cap = max(1, max(np.unique(row[ok & (owner == o)]).size for o in range(L.world)))
    grad = _nrm(np.random.default_rng(k), ids.shape[0], L.F * k)
    return L, ids, k, order, cap, grad, rng


def owner_expect(cs, dt=F64, ab=False):
    m = cs.m
    return ref_owner_fm(cs.recv, cs.lo, cs.n_owned, cs.shard, SHARD_ROWS, m.nd, m.k, m.w1, m.v, m.kfm, dt, ab)[0]


def owner_grad_expect(cs, dt=F64, ab=False):
    """rs_shard_owner_fm_grad as rs_capi.h states it: drows = g (w1_e + v_e . s - x_e |v_e|^2), dw1 = x^T g, dv =
    x^T (g s) - ((x^2)^T g) v over the owned columns.  (rows, drows, dw1, dv)"""
    m, f = cs.m, (np.abs if ab else (lambda t: t))
    x = ref_owner_rows(cs.recv, cs.n_owned, cs.shard, SHARD_ROWS, m.k, dt)
    col = m.nd + cs.lo * m.k + np.arange(cs.n_owned * m.k)
    w1, v = f(np.asarray(m.w1, dt)[col]), f(np.asarray(m.v, dt)[col])
    s, g, xx = f(np.asarray(cs.gs[:, :m.kfm], dt)), f(np.asarray(cs.gs[:, m.kfm], dt)), f(x)
    sgn = dt(1.0 if ab else -1.0)
    drows = g[:, None] * (w1[None, :] + s @ v.T + sgn * xx * (v * v).sum(1)[None, :])
    gx = g[:, None] * xx
    return x, drows, gx.sum(0), gx.T @ s + sgn * (gx * xx).sum(0)[:, None] * v


def combine_expect(cs, dt=F64):
    """(logit, s, g, loss, delta = the logit's bound SUM_TOL * sum |terms|)."""
    m = cs.m
    z, S = ref_combine(cs.part, cs.dense, m.nd, m.w0, m.w1, m.v, m.kfm, dt)
    g, loss = ref_bce(z, cs.labels, cs.scale, dt)
    absum = ref_combine(cs.part, cs.dense, m.nd, m.w0, m.w1, m.v, m.kfm, F64, ab=True)[0]
    return z, S, g, loss, SUM_TOL * absum


def check_combine(cs, z, S, g, loss, ref, q=1.0):
    """The comparison of rs_shard_fm_combine(_grad)'s outputs with `ref` = combine_expect(cs); q scales every bound."""
    rz, rS, rg, rl, delta = ref
    _sum_ok(z, rz, delta, "logit", factor=q)
    assert_scaled_close(S, rS, RTOL * q, "s")
    if g is not None:
        _sum_ok(g, rg, cs.scale * delta / 4 + 1e-5 * np.abs(rg), "g", factor=q)
    if loss is not None:
        _sum_ok(loss, rl, delta + 1e-5 * np.abs(rl), "loss", factor=q)


@pytest.mark.parametrize("c", DEDUP_CASES, ids=[c[0] for c in DEDUP_CASES])
def test_conditioning_dedup_grad(c):
    L, ids, k, order, cap, grad, _ = dedup_grad_inputs(c)
    slot = ref_dedup_route(ids, L, cap, order)[1]
    ref, written = ref_dedup_grad(grad, slot, L.world * cap)
    f32, _ = ref_dedup_grad(grad, slot, L.world * cap, F32)
    _sum_ok(f32[written], ref[written], ref_dedup_grad(grad, slot, L.world * cap, ab=True)[0][written], "dst",
            SUM_TOL / 4)


@pytest.mark.parametrize("c", OWNER_CASES, ids=[c[0] for c in OWNER_CASES])
def test_conditioning_owner_fm_and_grad(c):
    cs = owner_case(c)
    assert_scaled_close(owner_expect(cs, F32), owner_expect(cs), RTOL / 4, "partial records")
    if cs.n_owned and cs.m.k <= 16:
        ref, f32, ab = owner_grad_expect(cs), owner_grad_expect(cs, F32), owner_grad_expect(cs, ab=True)
        np.testing.assert_array_equal(f32[0], ref[0])
        assert_scaled_close(f32[1], ref[1], RTOL / 4, "drows")
        _sum_ok(f32[2], ref[2], ab[2], "dw1", SUM_TOL / 4)
        _sum_ok(f32[3], ref[3], ab[3], "dv", SUM_TOL / 4)


@pytest.mark.parametrize("c", COMBINE_CASES, ids=[_bid(c) for c in COMBINE_CASES])
def test_conditioning_combine(c):
    cs = combine_case(c)
    z, S, g, loss, _ = combine_expect(cs, F32)
    check_combine(cs, z, S, g, loss, combine_expect(cs), q=0.25)


@pytest.mark.parametrize("c", ROWS_FM_CASES, ids=[_bid(c) for c in ROWS_FM_CASES])
def test_conditioning_rows_fm(c):
    m, emb, dense = rows_fm_case(c)
    x = np.concatenate([dense, emb], 1)
    _sum_ok(ref_fm(x, m.w0, m.w1, m.v, F32), ref_fm(x, m.w0, m.w1, m.v), ref_fm(x, m.w0, m.w1, m.v, ab=True), "logit",
            SUM_TOL / 4)


# --------------------------------------------------------------------------
# B. GPU
# --------------------------------------------------------------------------
call, ptr = _lib.call, _lib.ptr


def _idev(a, dtype=I32):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype))).to("cuda")


def _ifull(n, v=ISENT):
    return torch.full((int(n),), v, dtype=torch.int32, device="cuda")


def _flag():
    return torch.zeros(1, dtype=torch.int32, device="cuda")


def _ids_dev(ids, pad):
    """(device ids with row stride F + pad, the stride); the padding holds garbage no field accepts."""
    ids = np.asarray(ids)
    junk = np.nan if ids.dtype == np.float32 else np.iinfo(ids.dtype).max - 3
    buf = np.full((ids.shape[0], ids.shape[1] + pad), junk, ids.dtype)
    buf[:, :ids.shape[1]] = ids
    return _idev(buf, ids.dtype), ids.shape[1] + pad


def _ldev(L):
    return SimpleNamespace(offs=_idev(L.offs, I64), vocab=_idev(L.vocab, I64), of=_idev(L.owner_fields, I32))


def _np(t):
    return t.detach().cpu().numpy()


def _fbuf(n, off=0, tail=8, fill=np.nan):
    """n floats `off` floats past a 16-B boundary: (the buffer, its view of n floats); head and tail hold SENT."""
    buf = torch.full((off + n + tail,), SENT, dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    buf[off:off + n] = fill
    return buf, buf[off:off + n]


def _untouched(buf, off, n):
    a = _np(buf)
    assert np.all(a[:off] == SENT) and np.all(a[off + n:] == SENT), "a kernel wrote outside its output"


def _ws(nbytes):
    return torch.zeros(max(int(nbytes), 256), dtype=torch.uint8, device="cuda")


def _bitwise(a, b):
    return np.array_equal(np.asarray(a).view(np.uint32) if np.asarray(a).dtype == np.float32 else a,
                          np.asarray(b).view(np.uint32) if np.asarray(b).dtype == np.float32 else b)


# ------------------------------------------------------------ rs_shard_bucketize
def _bucketize(L, D, ids, pad, flag=True):
    n = ids.size
    t, stride = _ids_dev(ids, pad)
    counts, perm, send, err = _ifull(L.world), _ifull(n), _ifull(n), _flag() if flag else None
    ws = _ws(_lib.lib().rs_shard_workspace_size(n, L.world))
    call("rs_shard_bucketize", ptr(t), KIND_OF[ids.dtype], stride, ptr(D.offs), ptr(D.vocab), L.F, ids.shape[0], L.rpr,
         L.world, ptr(counts), ptr(perm), ptr(send), ptr(ws), ptr(err), _lib.stream())
    return (counts, perm, send) + ((err,) if flag else ())


@pytest.mark.gpu
@pytest.mark.parametrize("c", BUCKET_CASES, ids=[_bid(c) for c in BUCKET_CASES])
def test_bucketize(gpu, c):
    L, ids = boundary_case(*c)
    D, pad = _ldev(L), 3 * (BUCKET_CASES.index(c) % 2)
    counts, perm, send, err = (_np(t) for t in _twice(lambda: _bucketize(L, D, ids, pad)))
    for got, ref in zip((counts, perm, send), ref_bucketize(ids, L)):
        np.testing.assert_array_equal(got, ref)
    assert err[0] == 0
    bad_ids, bad = with_bad(ids, L.vocab, np.random.default_rng(1))
    counts, perm, send, err = (_np(t) for t in _twice(lambda: _bucketize(L, D, bad_ids, pad)))
    assert err[0] == _lib.FLAG_BAD_ID
    np.testing.assert_array_equal(np.sort(perm), np.arange(ids.size))
    assert np.all(send[perm[bad]] == -1) and counts.sum() == ids.size
    for got, ref in zip((counts, perm, send), ref_bucketize(bad_ids, L)):
        np.testing.assert_array_equal(got, ref)
    for got, ref in zip(_bucketize(L, D, bad_ids, pad, flag=False), (counts, perm, send)):  # err_flag = NULL
        np.testing.assert_array_equal(_np(got), ref)


# ------------------------------------------------------------ rs_shard_slot_bucketize
def _slot_bucketize(L, D, ids, pad, cap, ws=None, flag=True, send=None):
    n = ids.size
    t, stride = _ids_dev(ids, pad)
    counts, slot, err, over = _ifull(L.world), _ifull(n), _flag() if flag else None, _flag()
    send = _ifull(L.world * cap, -1) if send is None else send
    ws = _ws(_lib.lib().rs_shard_workspace_size(n, L.world)) if ws is None else ws
    call("rs_shard_slot_bucketize", ptr(t), KIND_OF[ids.dtype], stride, ptr(D.offs), ptr(D.vocab), L.F, ids.shape[0],
         L.rpr, L.world, cap, ptr(counts), ptr(slot), ptr(send), ptr(ws), ptr(err), ptr(over), _lib.stream())
    return (counts, slot, send, over) + ((err,) if flag else ())


def _check_slots(got, ids, L, cap, send0=None):
    counts, slot, send, over = (_np(t) for t in got[:4])
    rc, rs, rsend, rover = ref_slot_bucketize(ids, L, cap, send0)
    np.testing.assert_array_equal(counts, rc)
    np.testing.assert_array_equal(slot, rs)
    np.testing.assert_array_equal(send, rsend)
    assert int(over[0] != 0) == int(rover)
    return rc


SLOT_CASES = [c for i, c in enumerate(BUCKET_CASES) if i % 2 == 0 or c[0] == 9_999_907]


@pytest.mark.gpu
@pytest.mark.parametrize("c", SLOT_CASES, ids=[_bid(c) for c in SLOT_CASES])
def test_slot_bucketize(gpu, c):
    """cap above, at and one below the largest owner's count: overflow below it alone, the overflowed lookups the
    reference's, unused send words keep their -1; then bad ids at a cap that fits the valid lookups exactly."""
    L, ids = boundary_case(*c)
    D, pad = _ldev(L), 3 * (BUCKET_CASES.index(c) % 2)
    top = int(ref_slot_bucketize(ids, L, 1)[0].max())
    for cap in (top + 1, top, top - 1):
        if cap >= 1:
            got = _twice(lambda: _slot_bucketize(L, D, ids, pad, cap))
            _check_slots(got, ids, L, cap)
            assert _np(got[4])[0] == 0 and (_np(got[3])[0] != 0) == (cap < top)
    bad_ids, bad = with_bad(ids, L.vocab, np.random.default_rng(1))
    top = max(1, int(ref_slot_bucketize(bad_ids, L, 1)[0].max()))
    got = _twice(lambda: _slot_bucketize(L, D, bad_ids, pad, top))
    _check_slots(got, bad_ids, L, top)
    assert _np(got[4])[0] == _lib.FLAG_BAD_ID and _np(got[3])[0] == 0, "a bad id took a position"
    assert np.all(_np(got[1])[bad] == -1)
    got2 = _slot_bucketize(L, D, bad_ids, pad, top, flag=False)  # err_flag = NULL
    for a, b in zip(got2, got[:4]):
        np.testing.assert_array_equal(_np(a), _np(b))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_slot_bucketize_bad_ids_take_no_position(gpu, dtype):
    """The defect this file settled: shard_owner answers (owner 0, local -1) for an out-of-range id, and the one-pass
    kernel ranked and counted it as owner 0's.  Owner 0 gets exactly cap valid lookups with bad ids in front of,
    between and behind them: counts[0] = cap, no overflow, every valid lookup has its slot."""
    L = layout([40, 60], 2, 50)
    rng = np.random.default_rng(4)
    B = 700  # two 1024-lookup blocks: the bad ids must stay out of the block totals too
    ids = np.stack([rng.integers(0, 40, B), rng.integers(10, 60, B)], 1).astype(dtype)  # field 0 -> owner 0
    ids[[0, 1, 350, 351, 698, 699], 0] = np.asarray([40, -1, 41, -1, 40, -1], dtype) if dtype != np.float32 else \
        np.asarray([40, -1, np.nan, -1, np.inf, -2], dtype)
    D = _ldev(L)
    rc = ref_slot_bucketize(ids, L, 1)[0]
    assert rc[0] == B - 6 and rc[1] == B
    got = _twice(lambda: _slot_bucketize(L, D, ids, 0, B))
    np.testing.assert_array_equal(_check_slots(got, ids, L, B), [B - 6, B])
    assert _np(got[3])[0] == 0 and _np(got[4])[0] == _lib.FLAG_BAD_ID
    L1 = layout([40], 2, 50)  # field 0 alone at cap = its valid lookups
    got = _slot_bucketize(L1, _ldev(L1), ids[:, :1].copy(), 0, B - 6)
    _check_slots(got, ids[:, :1], L1, B - 6)
    assert _np(got[3])[0] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1023, 1024, 1025, 300_000])
def test_slot_bucketize_block_counts(gpu, n):
    """One field: 1023 / 1024 / 1025 lookups (one block, one full block, two) and 300,000 (293 blocks: the
    look-back may pass its first 128-block window), at the exact capacity and one below."""
    L = layout([100_000], 5, 20_000)
    rng = np.random.default_rng(n)
    ids = rng.integers(0, 100_000, (n, 1)).astype(np.int32)
    D = _ldev(L)
    top = int(ref_slot_bucketize(ids, L, 1)[0].max())
    for cap in (top, top - 1):
        got = _twice(lambda: _slot_bucketize(L, D, ids, 0, cap))
        _check_slots(got, ids, L, cap)
        assert (_np(got[3])[0] != 0) == (cap < top) and _np(got[4])[0] == 0


@pytest.mark.gpu
def test_slot_bucketize_workspace_reuse(gpu):
    """Five calls on ONE workspace zeroed once, n and world changing, an rs_shard_bucketize call on the same
    workspace between two of them: the control word survives all of it."""
    rng = np.random.default_rng(9)
    shapes = [(5000, 3, 7), (300, 26, 64), (9000, 1, 2), (1, 1, 1), (2100, 5, 5)]
    lib = _lib.lib()
    ws = _ws(max(lib.rs_shard_workspace_size(B * F, w) for B, F, w in shapes))
    for i, (B, F, world) in enumerate(shapes):
        L = layout(rng.integers(1, 400, F), world)
        D = _ldev(L)
        ids = random_ids(rng, B, L.vocab, DTYPES[i % 3])
        top = int(ref_slot_bucketize(ids, L, 1)[0].max())
        _check_slots(_slot_bucketize(L, D, ids, 0, top, ws=ws), ids, L, top)
        if i == 2:
            t, stride = _ids_dev(ids, 0)
            counts, perm, send = _ifull(world), _ifull(ids.size), _ifull(ids.size)
            call("rs_shard_bucketize", ptr(t), KIND_OF[ids.dtype], stride, ptr(D.offs), ptr(D.vocab), F, B, L.rpr,
                 world, ptr(counts), ptr(perm), ptr(send), ptr(ws), None, _lib.stream())
            for got, ref in zip((counts, perm, send), ref_bucketize(ids, L)):
                np.testing.assert_array_equal(_np(got), ref)


# ------------------------------------------------------------ rs_shard_field_route / rs_shard_row_route
def _routes(L, D, ids, pad, S, R, flag=True):
    B = ids.shape[0]
    t, stride = _ids_dev(ids, pad)
    send_f, send_r, slot = _ifull(L.world * B * R), _ifull(L.world * B * S), _ifull(B * L.F)
    e1, e2 = (_flag(), _flag()) if flag else (None, None)
    call("rs_shard_field_route", ptr(t), KIND_OF[ids.dtype], stride, ptr(D.offs), ptr(D.vocab), L.F, B, L.rpr, L.world,
         ptr(D.of), S, R, ptr(send_f), ptr(e1), _lib.stream())
    call("rs_shard_row_route", ptr(t), KIND_OF[ids.dtype], stride, ptr(D.offs), ptr(D.vocab), L.F, B, L.rpr, L.world,
         ptr(D.of), S, ptr(send_r), ptr(slot), ptr(e2), _lib.stream())
    return (send_f, send_r, slot) + ((e1, e2) if flag else ())


def _check_routes(got, ids, L, S, R):
    send_f, send_r, slot = (_np(t) for t in got[:3])
    out, rslot = ref_field_route(ids, L, S)
    send_f = send_f.reshape(-1, R)
    np.testing.assert_array_equal(send_f[:, :S], out.reshape(-1, S))
    assert np.all(send_f[:, S:] == ISENT), "words past slot_stride were written"
    np.testing.assert_array_equal(send_r, out.reshape(-1))
    np.testing.assert_array_equal(slot, rslot.reshape(-1))


@pytest.mark.gpu
@pytest.mark.parametrize("c", ROUTE_CASES, ids=[c[0] for c in ROUTE_CASES])
def test_field_and_row_route(gpu, c):
    L, S, R, ids = route_case(c)
    D, pad = _ldev(L), 3 * (ROUTE_CASES.index(c) % 2)
    got = _twice(lambda: _routes(L, D, ids, pad, S, R))
    _check_routes(got, ids, L, S, R)
    assert _np(got[3])[0] == 0 and _np(got[4])[0] == 0
    clean_slot = _np(got[2])
    bad_ids, bad = with_bad(ids, L.vocab, np.random.default_rng(2))
    got = _twice(lambda: _routes(L, D, bad_ids, pad, S, R))
    _check_routes(got, bad_ids, L, S, R)
    assert _np(got[3])[0] == _lib.FLAG_BAD_ID and _np(got[4])[0] == _lib.FLAG_BAD_ID
    slot = _np(got[2])
    assert np.all(slot[bad] == -1) and np.array_equal(slot[~bad], clean_slot[~bad])
    for a, b in zip(_routes(L, D, bad_ids, pad, S, R, flag=False), got[:3]):  # err_flag = NULL
        np.testing.assert_array_equal(_np(a), _np(b))


# ------------------------------------------------------------ rs_gather_rows / rs_unpermute_rows / rs_scatter_rows
N_ROWS = 50


@pytest.mark.gpu
@pytest.mark.parametrize("c", GATHER_CASES, ids=[_bid(c) for c in GATHER_CASES])
def test_gather_unpermute_scatter_rows(gpu, c):
    k, n, ta, oa = c
    rng = np.random.default_rng(k * 1000 + n)
    table = _nrm(rng, N_ROWS, k)
    tbuf, tview = _fbuf(N_ROWS * k, ta)
    tview.copy_(_dev(table.reshape(-1)))
    assert (tview.data_ptr() % 16, tbuf.data_ptr() % 16) == (4 * ta % 16, 0)
    rows = np.where(rng.random(n) < 0.2, -1, rng.integers(0, N_ROWS, n)).astype(I32)
    bad_rows = rows.copy()
    bad_rows[rng.integers(0, n)] = -2
    bad_rows[rng.integers(0, n)] = N_ROWS

    def gather(r, flag=True):
        obuf, out = _fbuf(n * k, oa)
        err, r_t = _flag() if flag else None, _idev(r)
        call("rs_gather_rows", ptr(tview), N_ROWS, k, ptr(r_t), n, ptr(out), ptr(err), _lib.stream())
        _untouched(obuf, oa, n * k)
        return (out,) + ((err,) if flag else ())

    for r in (rows, bad_rows):
        out, err = _twice(lambda: gather(r))
        ref, flag = ref_gather(table, r, N_ROWS)
        assert _bitwise(_np(out).reshape(n, k), ref), gather_branch(k, n, 4 * ta, 4 * oa)
        assert _np(err)[0] == flag and flag == int(r is bad_rows)
    assert _bitwise(_np(gather(bad_rows, flag=False)[0]).reshape(n, k), ref_gather(table, bad_rows, N_ROWS)[0])
    # unpermute: dst[i] = src[perm[i]]
    src = _nrm(rng, n, k)
    sbuf, sview = _fbuf(n * k, ta)
    sview.copy_(_dev(src.reshape(-1)))
    perm = rng.permutation(n).astype(I32)
    perm_t = _idev(perm)

    def unpermute():
        dbuf, dst = _fbuf(n * k, oa)
        call("rs_unpermute_rows", ptr(sview), ptr(perm_t), k, n, ptr(dst), _lib.stream())
        _untouched(dbuf, oa, n * k)
        return (dst,)

    assert _bitwise(_np(_twice(unpermute)[0]).reshape(n, k), src[perm]), unpermute_branch(k, 4 * ta, 4 * oa)
    # scatter: src rows src_stride = F * k + 5 apart, negative slots skipped, untouched dst rows keep their NaN
    F = 5 if n % 5 == 0 else (3 if n % 3 == 0 else 1)
    B = n // F
    g = np.full((B, F * k + 5), np.nan, F32)
    g[:, :F * k] = _nrm(rng, B, F * k)
    slot = rng.permutation(n + 8)[:n].astype(I32)
    slot[rng.random(n) < 0.2] = -1
    slot[rng.integers(0, n)] = -5
    g_t, slot_t = _dev(g), _idev(slot)

    def scatter():
        dbuf, dst = _fbuf((n + 8) * k)
        call("rs_scatter_rows", ptr(g_t), F * k + 5, F, k, ptr(slot_t), B, ptr(dst), _lib.stream())
        _untouched(dbuf, 0, (n + 8) * k)
        return (dst,)

    got = _np(_twice(scatter)[0]).reshape(n + 8, k)
    ref = ref_scatter(g, slot, k, np.full((n + 8, k), np.nan, F32))
    assert np.array_equal(np.isnan(got), np.isnan(ref)) and _bitwise(np.nan_to_num(got), np.nan_to_num(ref))


# ------------------------------------------------------------ rs_shard_dedup_route / rs_shard_dedup_grad
def _dedup_route(L, D, ids, pad, cap, ws, flags=True):
    B = ids.shape[0]
    t, stride = _ids_dev(ids, pad)
    send, slot = _ifull(L.world * cap), _ifull(B * L.F)
    err, over = (_flag(), _flag()) if flags else (None, None)
    call("rs_shard_dedup_route", ptr(t), KIND_OF[ids.dtype], stride, ptr(D.offs), ptr(D.vocab), L.F, B, L.rpr, L.world,
         cap, ptr(send), ptr(slot), ptr(ws), ptr(err), ptr(over), _lib.stream())
    return (send, slot) + ((err, over) if flags else ())


def _dedup_grad(L, B, k, grad_t, gstride, slot_t, ws, cap):
    buf, dst = _fbuf(L.world * cap * k)
    call("rs_shard_dedup_grad", ptr(grad_t), gstride, L.F, k, B, L.world, ptr(slot_t), ptr(ws), ptr(dst),
         _lib.stream())
    _untouched(buf, 0, L.world * cap * k)
    return (dst,)


def _check_dedup(got, ids, L, cap, order, want_over):
    send, slot = _np(got[0]), _np(got[1])
    assert check_dedup_route(ids, L, cap, send, slot) == want_over
    rsend, rslot, rover = ref_dedup_route(ids, L, cap, order)  # the documented numbering, word for word
    np.testing.assert_array_equal(send, rsend)
    np.testing.assert_array_equal(slot, rslot)
    assert rover == want_over
    return slot


@pytest.mark.gpu
@pytest.mark.parametrize("c", DEDUP_CASES, ids=[c[0] for c in DEDUP_CASES])
def test_dedup_route_and_grad(gpu, c):
    """The route at cap = the largest distinct count (no overflow) and one below it (overflow, raised by the head
    lookup of the first row past the capacity), clean and with bad ids; after the clean and the bad route the
    gradient: only the slots of distinct rows written, each the sum over its row's lookups."""
    L, ids, k, order, cap, grad, rng = dedup_grad_inputs(c)
    B, D, pad = ids.shape[0], _ldev(L), 3 * (DEDUP_CASES.index(c) % 2)
    ws = _ws(_lib.lib().rs_shard_dedup_workspace_size(B * L.F, L.world))
    g_t = torch.full((B, L.F * k + 3), float("nan"), device="cuda")
    g_t[:, :L.F * k] = _dev(grad)
    bad_ids, bad = with_bad(ids, L.vocab, rng, 5)
    if c[6] in ("hot700", "hot1500", "chunks"):  # bad ids among the hot row's lookups, in lookup 0's 64-lookup group
        bad_ids[[3, 17, 40], 0] = np.asarray([-1, L.vocab[0], -1], ids.dtype)
        bad[[3 * L.F, 17 * L.F, 40 * L.F]] = True
    for these, flag in ((ids, 0), (bad_ids, _lib.FLAG_BAD_ID)):
        ok, row, owner, _ = rows_of(these, L)
        cap_now = max(1, max(np.unique(row[ok & (owner == o)]).size for o in range(L.world)))
        if these is ids and cap_now > 1:  # one below: overflow
            got = _twice(lambda: _dedup_route(L, D, these, pad, cap_now - 1, ws))
            _check_dedup(got, these, L, cap_now - 1, order, True)
            assert _np(got[2])[0] == 0 and _np(got[3])[0] != 0
        got = _twice(lambda: _dedup_route(L, D, these, pad, cap_now, ws))
        slot = _check_dedup(got, these, L, cap_now, order, False)
        assert _np(got[2])[0] == flag and _np(got[3])[0] == 0
        if these is bad_ids:
            assert np.all(slot[bad] == -1)
            for a, b in zip(_dedup_route(L, D, these, pad, cap_now, ws, flags=False), got[:2]):  # both flags NULL
                np.testing.assert_array_equal(_np(a), _np(b))
        dst = _np(_twice(lambda: _dedup_grad(L, B, k, g_t, L.F * k + 3, got[1], ws, cap_now))[0]).reshape(-1, k)
        ref, written = ref_dedup_grad(grad, slot, L.world * cap_now)
        assert np.array_equal(~np.isnan(dst).any(1), written) and np.array_equal(np.isnan(dst).all(1), ~written), \
            "a slot of no distinct row was written, or one of a distinct row was not"
        _sum_ok(dst[written], ref[written], ref_dedup_grad(grad, slot, L.world * cap_now, ab=True)[0][written],
                f"dst ({dedup_grad_branch(B, L.F, L.world, k)})")


@pytest.mark.gpu
def test_dedup_route_layout_flag(gpu):
    """The per-field path numbers field by field, so it needs increasing, disjoint row ranges: overlapping fields
    raise RS_FLAG_LAYOUT (beside RS_FLAG_BAD_ID when an id is bad too); disjoint ones do not."""
    for offs, bad_id, want in (([0, 5, 20], False, _lib.FLAG_LAYOUT), ([0, 10, 20], False, 0),
                               ([0, 9, 20], True, _lib.FLAG_LAYOUT | _lib.FLAG_BAD_ID)):
        L = layout([10, 10, 10], 2, 15, offs)
        ids = random_ids(np.random.default_rng(1), 40, L.vocab, I32)
        if bad_id:
            ids[7, 2] = 10
        ws = _ws(_lib.lib().rs_shard_dedup_workspace_size(ids.size, L.world))
        got = _dedup_route(L, _ldev(L), ids, 0, 40, ws)
        assert _np(got[2])[0] == want, offs


# ------------------------------------------------------------ the FM entries
def _prepared(m):
    """rs_fm_prepare's image of the WHOLE model, on a NaN-prefilled buffer."""
    n = _lib.lib().rs_fm_prepared_size(m.nd, m.F, m.k, m.kfm)
    assert n > 0
    prep, w1, v = torch.full((n,), float("nan"), device="cuda"), _dev(m.w1), _dev(m.v)  # (alive through the call)
    call("rs_fm_prepare", ptr(w1), ptr(v), m.nd, m.F, m.k, m.kfm, ptr(prep), _lib.stream())
    return prep


def _owner_fm(cs, prep, shard_t, recv, lo, n_owned, flag=True):
    m = cs.m
    buf = torch.full((cs.n_pairs, cs.pst), SENT, device="cuda")
    buf[:, :cs.P] = float("nan")
    err, recv_t = _flag() if flag else None, _idev(recv)
    call("rs_shard_owner_fm", ptr(recv_t), recv.shape[1], lo, n_owned, ptr(shard_t), SHARD_ROWS, m.nd, m.F, m.k,
         ptr(prep), m.kfm, ptr(buf), cs.pst, cs.n_pairs, ptr(err), _lib.stream())
    return (buf,) + ((err,) if flag else ())


def _records(buf, cs):
    """The kfm + 2 values of every partial record; the record's padding is 0, the stride's padding untouched."""
    a = _np(buf)
    assert np.all(a[:, cs.P:] == SENT), "floats past the record were written"
    assert np.all(a[:, cs.m.kfm + 2:cs.P] == 0), "the record's padding is not 0"
    return a[:, :cs.m.kfm + 2]


@pytest.mark.gpu
@pytest.mark.parametrize("c", OWNER_CASES, ids=[c[0] for c in OWNER_CASES])
def test_owner_fm(gpu, c):
    cs = owner_case(c)
    m, prep, shard_t = cs.m, _prepared(cs.m), _dev(cs.shard)
    branch = pipe_branch(m.nd, m.F, m.k, m.kfm, cs.n_owned) if cs.n_owned else "hipMemset2DAsync"
    buf, err = _twice(lambda: _owner_fm(cs, prep, shard_t, cs.recv, cs.lo, cs.n_owned))
    rec = _records(buf, cs)
    assert _np(err)[0] == 0
    if cs.n_owned == 0:
        assert np.all(rec == 0)
        return
    assert_scaled_close(rec, owner_expect(cs), RTOL, f"partial records ({branch})")
    # a local row = shard_rows: the flag, a zero row, every other pair bitwise unchanged
    cb = owner_case(c, bad=True)
    bbuf, berr = _twice(lambda: _owner_fm(cb, prep, shard_t, cb.recv, cb.lo, cb.n_owned))
    brec = _records(bbuf, cb)
    assert _np(berr)[0] == _lib.FLAG_BAD_ID
    assert_scaled_close(brec, owner_expect(cb), RTOL, f"partial records, bad row ({branch})")
    keep = np.arange(cs.n_pairs) != cs.n_pairs // 2
    assert _bitwise(brec[keep], rec[keep])
    assert _bitwise(_records(_owner_fm(cb, prep, shard_t, cb.recv, cb.lo, cb.n_owned, flag=False)[0], cb), brec)
    if branch.count(",") == 5:
        # launch_pipe4's constant shape against the generic kernel: the same fields as two owners of 13, summed
        halves = [_records(_owner_fm(cs, prep, shard_t, np.ascontiguousarray(cs.recv[:, h:h + 13]), cs.lo + h, 13)[0],
                           cs).astype(F64) for h in (0, 13)]
        assert pipe_branch(m.nd, m.F, m.k, m.kfm, 13) == "shard_fm_pipe<4,1,16,1>"
        assert_scaled_close(rec, halves[0] + halves[1], RTOL, "constant shape against the generic kernel")
        assert_scaled_close(halves[0] + halves[1], owner_expect(cs), RTOL, "the generic kernel's halves")


GRAD_CASES = [c for c in OWNER_CASES if c[1] > 0 and c[5] <= 16]


@pytest.mark.gpu
@pytest.mark.parametrize("c", GRAD_CASES, ids=[c[0] for c in GRAD_CASES])
def test_owner_fm_grad(gpu, c):
    cs = owner_case(c)
    m, w = cs.m, cs.n_owned * cs.m.k
    gst = m.kfm + 1 + 3 * (GRAD_CASES.index(c) % 2)
    gs = torch.full((cs.n_pairs, gst), float("nan"), device="cuda")
    gs[:, :m.kfm + 1] = _dev(cs.gs)
    shard_t, recv_t, w1_t, v_t = _dev(cs.shard), _idev(cs.recv), _dev(m.w1), _dev(m.v)

    def run():
        bufs = [_fbuf(cs.n_pairs * w), _fbuf(cs.n_pairs * w), _fbuf(w), _fbuf(w * m.kfm)]
        call("rs_shard_owner_fm_grad", ptr(recv_t), cs.recv.shape[1], cs.lo, cs.n_owned, ptr(shard_t), SHARD_ROWS, m.nd,
             m.k, ptr(w1_t), ptr(v_t), m.kfm, ptr(gs), gst, cs.n_pairs, *[ptr(v) for _, v in bufs], _lib.stream())
        for (b, v) in bufs:
            _untouched(b, 0, v.numel())
        return tuple(v for _, v in bufs)

    rows, drows, dw1, dv = (_np(t) for t in _twice(run))
    ref, ab = owner_grad_expect(cs), owner_grad_expect(cs, ab=True)
    assert _bitwise(rows.reshape(cs.n_pairs, w), ref[0].astype(F32))
    assert_scaled_close(drows.reshape(cs.n_pairs, w), ref[1], RTOL, "drows")
    _sum_ok(dw1, ref[2], ab[2], "dw1")
    _sum_ok(dv.reshape(w, m.kfm), ref[3], ab[3], "dv")


def _combine_inputs(cs, pst):
    m = cs.m
    part = torch.full((cs.world * cs.B, pst), float("nan"), device="cuda")
    part[:, :cs.P] = _dev(cs.part.reshape(-1, cs.P))
    dense = torch.full((cs.B, m.nd + 2), float("nan"), device="cuda")
    dense[:, :m.nd] = _dev(cs.dense)
    return part, dense


@pytest.mark.gpu
@pytest.mark.parametrize("c", COMBINE_CASES, ids=[_bid(c) for c in COMBINE_CASES])
def test_combine_and_combine_grad(gpu, c):
    cs = combine_case(c)
    m, pst = cs.m, cs.P + 3 * (COMBINE_CASES.index(c) % 2)
    prep, w0, labels = _prepared(m), _dev(m.w0), _dev(cs.labels)
    part, dense = _combine_inputs(cs, pst)

    def fwd():
        buf, logit = _fbuf(cs.B)
        call("rs_shard_fm_combine", ptr(part), pst, cs.world, cs.B, ptr(dense) if m.nd else None, m.nd + 2, m.nd, m.F,
             m.k, ptr(prep), ptr(w0), m.kfm, ptr(logit), _lib.stream())
        _untouched(buf, 0, cs.B)
        return (logit,)

    def grad():
        (b1, logit), (b2, loss) = _fbuf(cs.B), _fbuf(cs.B)
        gs = torch.full((cs.B, cs.gst), SENT, device="cuda")
        gs[:, :m.kfm + 1] = float("nan")
        call("rs_shard_fm_combine_grad", ptr(part), pst, cs.world, cs.B, ptr(dense) if m.nd else None, m.nd + 2, m.nd,
             m.F, m.k, ptr(prep), ptr(w0), m.kfm, ptr(labels), cs.scale, ptr(logit), ptr(gs), cs.gst,
             ptr(loss) if cs.loss else None, _lib.stream())
        _untouched(b1, 0, cs.B)
        _untouched(b2, 0, cs.B)
        return logit, gs, loss

    ref = combine_expect(cs)
    z = _np(_twice(fwd)[0])
    z2, gs, loss = (_np(t) for t in _twice(grad))
    assert _bitwise(z, z2), "the training combine's logit is not the forward's"
    assert np.all(gs[:, m.kfm + 1:] == SENT)
    assert cs.loss or np.all(np.isnan(loss)), "loss = NULL, yet something was written"
    check_combine(cs, z, gs[:, :m.kfm], gs[:, m.kfm], loss if cs.loss else None, ref)


# ------------------------------------------------------------ rs_shard_fm_pipe
@pytest.mark.gpu
def test_pipe_equals_its_three_parts(gpu):
    """For each non-empty combination of {prev, cur, nxt}: send and logit_prev are bitwise what rs_shard_fm_combine,
    rs_shard_owner_fm and rs_shard_field_route write into the same fused records [row ids | partial].  An absent
    route leaves the row-id words alone, an absent combine the logits; the entry has no "no owner part": n_owned =
    0 zeroes the partial words, as rs_shard_owner_fm does.  And one empty-batch call."""
    rng = np.random.default_rng(11)
    L = layout([9, 30, 4, 17, 25, 6, 12], 3)
    D, W, B, rank = _ldev(L), 3, 17, 1
    m = fm_params(rng, 5, L.F, 8, 10)
    P, S = partial_width(m.kfm), L.slot_stride
    R = S + P
    lo, n_owned = (int(x) for x in L.owner_fields[rank])
    assert n_owned > 0
    prep, w0 = _prepared(m), _dev(m.w0)
    shard = _dev(_nrm(rng, L.rpr, m.k) * 0.5)
    # recv: what the three requesters sent this owner (row ids) and what the owners answered (partials of batch t-1)
    recv = np.zeros((W * B, R), I32)
    for q in range(W):
        recv[q * B:(q + 1) * B, :S] = ref_field_route(random_ids(rng, B, L.vocab), L, S)[0][rank]
    recv[:, S:] = (_nrm(rng, W * B, P) * 0.3).astype(F32).view(I32)
    recv_t = _idev(recv)
    dense = _dev(rng.random((B, m.nd)))
    ids_next, stride = _ids_dev(random_ids(rng, B, L.vocab, I32), 3)
    st = _lib.stream()

    def parts(n_own):
        send, (lb, logit), err = _ifull(W * B * R), _fbuf(B), _flag()
        call("rs_shard_owner_fm", ptr(recv_t), R, lo, n_own, ptr(shard), L.rpr, m.nd, m.F, m.k, ptr(prep), m.kfm,
             ptr(send) + 4 * S, R, W * B, ptr(err), st)
        call("rs_shard_field_route", ptr(ids_next), _lib.ID_I32, stride, ptr(D.offs), ptr(D.vocab), L.F, B, L.rpr, W,
             ptr(D.of), S, R, ptr(send), ptr(err), st)
        call("rs_shard_fm_combine", ptr(recv_t) + 4 * S, R, W, B, ptr(dense), m.nd, m.nd, m.F, m.k, ptr(prep), ptr(w0),
             m.kfm, ptr(logit), st)
        assert _np(err)[0] == 0
        return _np(send).reshape(-1, R), _np(logit)

    def pipe(prev, cur, nxt, batch=B):
        send, (lb, logit), err = _ifull(W * B * R), _fbuf(B), _flag()
        call("rs_shard_fm_pipe", ptr(recv_t), lo, n_owned if cur else 0, ptr(shard), L.rpr,
             ptr(dense) if prev else None, m.nd, ptr(logit) if prev else None, ptr(ids_next) if nxt else None,
             _lib.ID_I32, stride, ptr(D.offs), ptr(D.vocab), L.rpr, ptr(D.of), S, ptr(send), W, batch, m.nd, L.F, m.k, ptr(prep), ptr(w0), m.kfm,
             ptr(err), st)
        _untouched(lb, 0, B)
        assert _np(err)[0] == 0
        return send, logit

    full, zero = parts(n_owned), parts(0)
    assert np.all(zero[0][:, S:] == 0) and not np.all(full[0][:, S:] == 0)
    for prev in (False, True):
        for cur in (False, True):
            for nxt in (False, True):
                if not (prev or cur or nxt):
                    continue
                send, logit = (_np(t) for t in _twice(lambda: pipe(prev, cur, nxt)))
                send, want = send.reshape(-1, R), (full if cur else zero)
                assert np.array_equal(send[:, S:], want[0][:, S:]), (prev, cur, nxt)
                assert np.array_equal(send[:, :S], want[0][:, :S] if nxt else np.full((W * B, S), ISENT)), \
                    (prev, cur, nxt)
                assert _bitwise(logit, want[1]) if prev else np.all(np.isnan(logit)), (prev, cur, nxt)
    send, logit = pipe(True, True, True, batch=0)  # an empty batch: nothing launched, nothing written
    assert np.all(_np(send) == ISENT) and np.all(np.isnan(_np(logit)))


# ------------------------------------------------------------ rs_rows_fm_fwd
@pytest.mark.gpu
@pytest.mark.parametrize("c", ROWS_FM_CASES, ids=[_bid(c) for c in ROWS_FM_CASES])
def test_rows_fm_fwd(gpu, c):
    m, emb, dense = rows_fm_case(c)
    B = emb.shape[0]
    prep, w0, emb_t = _prepared(m), _dev(m.w0), _dev(emb)
    dense_t = torch.full((B, m.nd + 2), float("nan"), device="cuda")
    dense_t[:, :m.nd] = _dev(dense)

    def run():
        buf, logit = _fbuf(B)
        call("rs_rows_fm_fwd", ptr(emb_t), ptr(dense_t) if m.nd else None, m.nd + 2, m.nd, m.F, m.k, ptr(prep), ptr(w0),
             m.kfm, ptr(logit), B, _lib.stream())
        _untouched(buf, 0, B)
        return (logit,)

    x = np.concatenate([dense, emb], 1)
    _sum_ok(_np(_twice(run)[0]), ref_fm(x, m.w0, m.w1, m.v), ref_fm(x, m.w0, m.w1, m.v, ab=True), "logit")
