"""The fused MLP tower (mlp.hip, mlp_tower.hpp) and the one-launch model
forwards built on it (rs_deepfm_fwd / _hm, rs_dcn_fwd / _hm,
rs_din_forward_ids), one entry point at a time through the C ABI, against
plain numpy float64 restatements, at every shape where a launcher or a kernel
takes another branch.

Part A (CPU): the references are pinned to the oracle's functions (1e-12) and
to a hand-computed tower; the launchers' dispatch (mlp_geom, mlp_tail_ok,
mlp_slices, fm_geom, cross_geom, deepfm_ws_ok / deepfm_all_ok, the DCN chain,
din_tower_ok) is restated in Python, so every GPU case below is (shape,
options) -> the name of the branch it takes, computed and not typed; every
launch line of mlp_run, launch_deepfm, dcn_run and launch_din_tower is named
by a case; the restated "supported" predicates equal the library's host
queries on both sides of every bound; the bound shapes are derived and their
neighbours refused through the real entries; and every GPU case is
conditioned: the same restatement in float32 numpy sits within RTOL / 4 of the
float64 one under the comparison used on the GPU.

Part B (GPU): padded strides (NaN in the input padding, a sentinel in the
output padding), NaN-prefilled outputs and prepared buffers, every call twice
on fresh outputs for bitwise equality, ids as int32 / int64 / float32, a clean
run (flag 0) and runs with one out-of-range id (flag raised, zero row, the
other samples bitwise unchanged), err_flag = NULL where rs_capi.h allows it
(flag_error tests the pointer), every option restored in a finally.

Inputs keep the references O(1): embedding rows N(0,1) * 0.5, dense features
U[0,1), Dense kernels N(0,1) / sqrt(fan_in), biases N(0,1) * 0.1, FM v
N(0,1) / sqrt(d), CrossNet w N(0,1) * 0.05 / sqrt(d) (|alpha_L| < 10 asserted).

Tolerances: the project's contract, no new number.  Post-sigmoid outputs:
helpers.assert_rel_close at 1e-5; raw tower outputs and logits:
helpers.assert_scaled_close at 1e-5.  The FM logit cancels (0.5 ((x v)^2 -
x^2 v^2) beside the linear term): it is bounded by SUM_TOL * sum |terms| from
the reference on absolute values; an fp32 sum of n terms is off by at most
about n eps sum |terms| / 2 in the worst order and by sqrt(n) eps sum |terms|
typically, 1e-6 sum |terms| at the n ~ 500 columns of these shapes, and
SUM_TOL = 2e-6 is the bound the block tests use for such sums.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from oracle import ctr_oracle as O
from recommender_system_amd import _lib
from tests.helpers import RTOL, assert_rel_close, assert_scaled_close
from tests.test_train_blocks import F32, F64, SENT, SUM_TOL, _d, _dev, _get, _nrm, _out, _p, _refused, _rows, _twice

torch = pytest.importorskip("torch")

ACTS = ("linear", "relu", "prelu", "sigmoid")  # RS_ACT_NONE .. RS_ACT_SIGMOID = 0 .. 3
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "recommender_system_amd", "csrc")
KINDS = ((np.int32, _lib.ID_I32), (np.int64, _lib.ID_I64), (np.float32, _lib.ID_F32))
BATCHES = (1, 15, 16, 17, 33, 49)  # around the 16-row tile (and DIN's 8 samples per workgroup)


# --------------------------------------------------------------------------
# References.  dt = float64: the reference; dt = float32: the conditioning run.
# --------------------------------------------------------------------------
def _sig(z):
    return 1.0 / (1.0 + np.exp(-z))


def _act(z, act, alpha):
    if act == "relu":
        return np.maximum(z, 0)
    if act == "prelu":
        return np.maximum(z, 0) + alpha * np.minimum(z, 0)
    if act == "sigmoid":
        return _sig(z)
    return z


def ref_tower(x, layers, acts, in_scale=None, in_shift=None, head=0, extra=None, c0=1.0, c1=1.0, dt=F64):
    """rs_mlp_fwd / rs_mlp_affine_fwd: layers [(W [K, N], bias | None, alpha | None)], acts[l] in 0..3; a missing
    bias / alpha is 0; head 1: sigmoid(c0 * tower[:, 0] + c1 * extra)."""
    h = np.asarray(x, dt)
    if in_scale is not None:
        h = h * np.asarray(in_scale, dt) + np.asarray(in_shift, dt)
    for (W, b, al), a in zip(layers, acts):
        z = h @ np.asarray(W, dt)
        if b is not None:
            z = z + np.asarray(b, dt)
        h = _act(z, ACTS[a], dt(0) if al is None else np.asarray(al, dt))
    if not head:
        return h
    z = dt(c0) * h[:, 0]
    if extra is not None:
        z = z + dt(c1) * np.asarray(extra, dt).reshape(-1)
    return _sig(z)


def ref_fm(x, w0, w1, v, dt=F64, ab=False):
    """FMLayer on x [B, d]: w0 + x w1 + 0.5 sum_f ((x v)_f^2 - (x^2 v^2)_f); ab: its sum |terms|."""
    x, w1, v = np.asarray(x, dt), np.asarray(w1, dt).reshape(-1), np.asarray(v, dt)
    w0 = dt(np.asarray(w0).reshape(-1)[0])
    if ab:
        x, w1, v, w0 = np.abs(x), np.abs(w1), np.abs(v), abs(w0)
        return w0 + x @ w1 + dt(0.5) * (((x @ v) ** 2).sum(1) + ((x ** 2) @ (v ** 2)).sum(1))
    return w0 + x @ w1 + dt(0.5) * (((x @ v) ** 2).sum(1) - ((x ** 2) @ (v ** 2)).sum(1))


def _gather(table, ids, vocab, dt=F64):
    """Rows of the concatenated table [B, F, k]; an out-of-range id reads a zero row."""
    table, ids, vocab = np.asarray(table, dt), np.asarray(ids, np.int64), np.asarray(vocab, np.int64)
    offs = np.concatenate([[0], np.cumsum(vocab)[:-1]]).astype(np.int64)
    ok = (ids >= 0) & (ids < vocab[None, :])
    return table[np.where(ok, offs[None, :] + ids, 0)] * ok[:, :, None]


def _x_of(dense, ids, vocab, table, dt=F64):
    """[dense | EmbedLayer(ids)]: the Keras column order."""
    e = _gather(table, ids, vocab, dt)
    return np.concatenate([np.asarray(dense, dt).reshape(e.shape[0], -1), e.reshape(e.shape[0], -1)], 1)


def ref_deepfm(x, w0, w1, v, layers, acts, c0, c1, dt=F64):
    """DeepFM.call on x = [dense | rows]: (sigmoid(c0 dnn + c1 fm), fm)."""
    fm = ref_fm(x, w0, w1, v, dt)
    return ref_tower(x, layers, acts, head=1, extra=fm, c0=c0, c1=c1, dt=dt), fm


def ref_cross(x0, W, b, dt=F64):
    """CrossLayer: x_{l+1} = x0 (x_l . w_l) + b_l + x_l; (x_L, the alpha_L of x_L = alpha_L x0 + sum b_l)."""
    x0, W, b = np.asarray(x0, dt), np.asarray(W, dt), np.asarray(b, dt)
    x, alpha, beta = x0, np.ones(x0.shape[0], dt), np.zeros(x0.shape[1], dt)
    for l in range(W.shape[0]):
        alpha = alpha * (1 + x0 @ W[l]) + beta @ W[l]
        beta = beta + b[l]
        x = x0 * (x @ W[l])[:, None] + b[l] + x
    return x, alpha


def ref_dcn(x, cw, cb, layers, acts, out_kernel, out_bias, dt=F64):
    """DCN.call on x: sigmoid(Dense1([CrossNet(x) | tower(x)])); (y, alpha_L)."""
    xl, alpha = ref_cross(x, cw, cb, dt)
    deep = ref_tower(x, layers, acts, dt=dt)
    z = np.concatenate([xl, deep], 1) @ np.asarray(out_kernel, dt).reshape(-1) + dt(np.asarray(out_bias).reshape(-1)[0])
    return _sig(z), alpha


MASKED = -2.0 ** 32  # the reference's -2**32 + 1 in fp32


def ref_din(hist, cand, table, att, other, in_scale, in_shift, layers, acts, dt=F64):
    """rs_din_forward_ids as rs_capi.h states it: key = value = table[hist], query = table[cand], mask = hist != 0,
    e_t = [q, key, q - key, q key], two Dense + PReLU (alpha per position), Dense(1), masked softmax, pooled =
    weights @ values; then the tower over [pooled | cand rows | other] * in_scale + in_shift.  An id outside
    [0, vocab) reads a zero row.  att = (W1, b1, alpha1 [T, H1], W2, b2, alpha2 [T, H2], w3, b3).  (y, pooled)."""
    table = np.asarray(table, dt)
    V = table.shape[0]
    hist, cand = np.asarray(hist, np.int64), np.asarray(cand, np.int64).reshape(-1)
    row = lambda i: table[np.where((i >= 0) & (i < V), i, 0)] * ((i >= 0) & (i < V))[..., None]
    keys, q = row(hist), row(cand)
    W1, b1, a1, W2, b2, a2, w3, b3 = (np.asarray(t, dt) for t in att)
    qb = np.broadcast_to(q[:, None, :], keys.shape)
    h = np.concatenate([qb, keys, qb - keys, qb * keys], -1)
    h = _act(h @ W1 + b1, "prelu", a1[None])
    h = _act(h @ W2 + b2, "prelu", a2[None])
    s = h @ w3.reshape(-1) + b3.reshape(-1)[0]
    s = np.where(hist == 0, dt(MASKED), s)
    e = np.exp(s - s.max(1, keepdims=True))
    pooled = np.einsum("bt,btk->bk", e / e.sum(1, keepdims=True), keys)
    x = np.concatenate([pooled, q, np.asarray(other, dt).reshape(len(cand), -1)], 1)
    return ref_tower(x, layers, acts, in_scale, in_shift, dt=dt)[:, 0], pooled


# --------------------------------------------------------------------------
# The launchers' dispatch, restated (mlp_tower.hpp, mlp.hip, embed_fm.hpp,
# deepfm.hip, cross.hip, din.hip)
# --------------------------------------------------------------------------
def rup(v, m):
    return (v + m - 1) // m * m


def mlp_geom(dims):
    """mlp_geom: None when refused, else Kp, Np, ptot, total (floats), rs (floats), lds (bytes)."""
    L = len(dims) - 1
    if L < 1 or L > 8 or any(d < 1 for d in dims):
        return None
    Kp, Np = [rup(d, 16) for d in dims[:-1]], [rup(d, 16) for d in dims[1:]]
    if max(Kp + Np) > 1024:
        return None
    ptot = 2 * sum(Np)
    rs = rup(max(Kp + Np), 64) + 8
    lds = (32 * rs + 16 * 256 + ptot) * 4
    if lds > 160 * 1024:
        return None
    return dict(L=L, K=list(dims[:-1]), N=list(dims[1:]), Kp=Kp, Np=Np, ptot=ptot, rs=rs, lds=lds,
                total=sum(k * n for k, n in zip(Kp, Np)) + ptot)


def mlp_slices(T, G, NW=16):
    if T >= 4:
        return 1
    return max(1, min(NW // T, G))


def mlp_tail_ok(g, l0=1):
    """mlp_tail_ok: (gwa, gwb) when the layers after l0's caller-run layer are two split layers and a one-unit head
    (+ at most one 1 -> 1 layer) of an accepted (gwa, gwb), else None."""
    L, N, Np, Kp = g["L"], g["N"], g["Np"], g["Kp"]
    if L < l0 + 3:
        return None
    extra = L == l0 + 4 and N[L - 2] == 1 and N[L - 1] == 1 and Kp[L - 1] == 16
    if (L != l0 + 3 and not extra) or N[l0 + 2] != 1:
        return None
    gw = []
    for l in (l0, l0 + 1):
        T, G = Np[l] >> 4, Kp[l] >> 4
        if T < 1 or T > 16 or 16 % T or G % (16 // T):
            return None
        gw.append(G // (16 // T))
    return tuple(gw) if tuple(gw) in ((8, 2), (4, 2), (8, 4), (4, 1)) else None


def _tail82(g):
    return g["L"] >= 4 and mlp_tail_ok(g) == (8, 2)


def tower_features(g, l0=0, lstop=8):
    """What mlp_tower_tile does on layers l0 .. : the folded head (fhead) and, per layer run, (T, G, S)."""
    L, LH = g["L"], g["L"] - 1
    fhead = lstop >= L and LH - 1 >= l0 and g["N"][LH] == 1 and \
        mlp_slices(g["Np"][LH - 1] >> 4, g["Kp"][LH - 1] >> 4) == 1
    lrun = LH if fhead else min(lstop, L)
    return fhead, [(g["Np"][l] >> 4, g["Kp"][l] >> 4, mlp_slices(g["Np"][l] >> 4, g["Kp"][l] >> 4))
                   for l in range(l0, lrun)]


def tail_features(g):
    """The sub-branches of a tower that takes the split-K tail after layer 0."""
    f = ["layer0_tiles" if g["Np"][0] == 256 else "tower_tile(0,1)",
         "tail<8,2,8,4>" if (g["Np"][1], g["Np"][2]) == (128, 64) else "tail<8,2>"]
    if g["L"] == 5:
        f.append("extra 1->1")
    return f


def tower_branch(dims, pieces=False):
    """mlp_run: (the kernel launched, the sub-branches its body takes)."""
    g = mlp_geom(dims)
    name = "mlp_tower_pc" if pieces else "mlp_tower"
    if _tail82(g):
        return name + "<16,true>", tail_features(g)
    fhead, layers = tower_features(g)
    f = ["fhead"] if fhead else []
    f += sorted({"S>1" if S > 1 else ("T>16 (a wave's second item)" if T > 16 else "S=1") for T, G, S in layers})
    return name + "<16>", f


def fm_geom(nd, F, k, kfm):
    ok = (F == 0 or k in (4, 8, 16, 32, 64)) and 1 <= kfm <= 31
    return dict(mfma=ok, KV=(4 if F == 0 else k // 4), NT=(kfm + 1 + 15) // 16, DB=(nd + 3) // 4) if ok else \
        dict(mfma=False)


def deepfm_supported(nd, F, k, kfm, dims):
    if nd < 0 or F < 1 or F > 128 or kfm < 1 or k not in (8, 16):
        return False
    fg = fm_geom(nd, F, k, kfm)
    if not fg["mfma"] or fg["NT"] != 1:
        return False
    g = mlp_geom(dims)
    return bool(g) and dims[0] == nd + F * k and dims[-1] == 1 and g["lds"] <= 120 * 1024


def deepfm_branch(nd, F, k, kfm, dims, hm_entry, opt):
    """launch_deepfm (deepfm_ws_ok, deepfm_all_ok, the ka / generic choice): the kernel launched."""
    fg, g = fm_geom(nd, F, k, kfm), mlp_geom(dims)
    hm, KV, DB = hm_entry and F <= 32, fg["KV"], fg["DB"]
    if KV == 4:
        shape = hm and F == 26 and g["L"] >= 2 and g["Np"][0] == 256 and g["Kp"][0] == 16 * (F + 1)
        if shape and 1 <= nd <= 16 and DB <= 4 and g["ptot"] <= 1024 and opt >= 2:
            if _tail82(g):
                return "deepfm_all<27,4,8,2>" if opt == 3 else "deepfm_all<27,3,8,2>"
            return "deepfm_all<27,3>"
        if shape and 13 <= nd <= 16 and DB == 4 and (g["Np"][1] >> 4) >= 8 and opt == 0:
            return "deepfm_ws<27,8,2>" if _tail82(g) else "deepfm_ws<27>"
    if hm and F <= 32 and DB <= 16:
        return f"deepfm_fused_ka<{KV}>"
    return f"deepfm_fused<{KV}>"


def cross_geom(d, L):
    return dict(NT=(L + 15) // 16, DB=(d + 3) // 4)


def kernarg_meta(hm_entry, F, k):
    return hm_entry and k == 16 and 1 <= F <= 32


def dcn_supported(nd, F, k, n_cross, dims):
    if nd < 0 or F < 1 or F > 128 or k < 4 or k % 4 or n_cross < 0 or n_cross > 31:
        return False
    g = mlp_geom(dims)
    return bool(g) and dims[0] == nd + F * k and dims[-1] == 1 and g["lds"] <= 100 * 1024


def dcn_branch(nd, F, k, n_cross, dims, hm_entry, opt):
    """dcn_run's chain: the kernel launched."""
    g, NT = mlp_geom(dims), cross_geom(nd + F * k, n_cross + 1)["NT"]
    hm, reg = kernarg_meta(hm_entry, F, k), opt == 0
    if hm and NT == 1 and _tail82(g):
        return "dcn_fused_ka<1,true,true>" if reg else "dcn_fused_ka<1,true>"
    if hm and NT == 1:
        return "dcn_fused_ka<1,false,true>" if reg else "dcn_fused_ka<1>"
    if hm:
        return "dcn_fused_ka<2>"
    return f"dcn_fused<{NT}>"


def din_layout(T, k, H1, H2):
    """din_geom's tile counts and df_layout (floats)."""
    NTT, HT1, HT2, KS = (T + 15) // 16, (H1 + 15) // 16, (H2 + 15) // 16, k // 4
    a2 = NTT * 16 * (HT1 * 16 + 4)
    w2 = a2 + NTT * 16 * (HT2 * 16 + 4)
    w1 = w2 + HT2 * HT1 * 64 * 4
    part = w1 + 3 * HT1 * KS * 64
    return dict(NTT=NTT, HT1=HT1, HT2=HT2, KS=KS, part=part, total=part + 8 * NTT * (2 + 16))


DIN_STATIC = 1024 + 8 * (128 + 2) * 8  # din.hip: the static bias / w3 tiles and the id tile


def din_tower(T, k, H1, H2, dims):
    """din_tower_ok: None when the fused launch is refused, else (tbase, lds bytes, NTT)."""
    if T < 1 or T > 1024 or k not in (4, 8, 16) or not 1 <= H1 <= 128 or not 1 <= H2 <= 64:
        return None
    lay = din_layout(T, k, H1, H2)
    df = lay["total"] * 4 if lay["NTT"] * 16 <= 128 and lay["total"] * 4 + DIN_STATIC <= 160 * 1024 else 0
    if lay["HT1"] != 5 or lay["HT2"] != 3 or not df:
        return None
    g = mlp_geom(dims)
    if not g or dims[0] > 64 or dims[0] < 2 * k or g["Np"][0] != 256 or not _tail82(g):
        return None
    tfl = 32 * g["rs"] + 16 * 256 + g["ptot"]
    tbase = 0 if tfl <= lay["part"] else lay["total"]
    lds = max(df, (tbase + tfl) * 4)
    return (tbase, lds, lay["NTT"]) if lds + DIN_STATIC <= 160 * 1024 else None


def din_branch(T, k, H1, H2, dims):
    """launch_din_tower: the kernel launched and the LDS layout din_tower_ok picked."""
    tbase, _, NTT = din_tower(T, k, H1, H2, dims)
    KS = k // 4
    return (f"din_fused_tower<{KS},5,3,7>" if KS == 2 and NTT == 7 else f"din_fused_tower<{KS},5,3>",
            "tbase=0" if tbase == 0 else "tbase=total")


# --------------------------------------------------------------------------
# The GPU cases (inputs are drawn from each case's own seed, on the CPU)
# --------------------------------------------------------------------------
def _layers(rng, dims, acts, no_bias=(), no_alpha=()):
    """[(W, bias | None, alpha | None)]: N(0,1)/sqrt(K), N(0,1)*0.1, N(0,1)*0.5.  alpha is given for every PReLU layer
    and (to show it is ignored) for every second other layer."""
    out = []
    for l, (K, N) in enumerate(zip(dims[:-1], dims[1:])):
        W = _nrm(rng, K, N) / F32(np.sqrt(K))
        b = None if l in no_bias else _nrm(rng, N) * F32(0.1)
        al = _nrm(rng, N) * F32(0.5) if (acts[l] == 2 and l not in no_alpha) else None
        out.append((W, b, al))
    return out


MIX = (1, 2, 3, 0, 2, 1, 3, 0)  # relu, prelu, sigmoid, linear, ..: the four activations within one tower


def _t(name, dims, acts=None, head=0, extra=False, mode="plain", M=None, **kw):
    L = len(dims) - 1
    acts = list(MIX[:L - 1]) + [0] if acts is None else list(acts)
    return dict(name=name, dims=list(dims), acts=acts, head=head, extra=extra, mode=mode, M=M, **kw)


TOWER_CASES = [_t(f"in{w}", [w, 40, 5]) for w in (1, 15, 16, 17, 1008, 1024)] + \
              [_t(f"hid{w}", [40, w, 5]) for w in (1, 15, 16, 17, 1008, 1024)] + [
    _t("L1", [17, 5], acts=[2]),
    _t("L1 head", [64, 1], acts=[0], head=1, extra=True),
    _t("L8 mixed", [20, 33, 16, 70, 17, 48, 15, 64, 3], acts=list(MIX)),
    _t("L8 head", [31, 64, 64, 32, 96, 64, 80, 64, 1], head=1, extra=True),
    # the four (8, 2) tail families, exact and padded, and NFM's extra 1 -> 1 layer
    _t("tail 256-128-64", [37, 256, 128, 64, 1], acts=[1, 1, 1, 0], head=1, extra=True),
    _t("tail 250-120-60", [37, 250, 120, 60, 1], acts=[2, 1, 3, 0], head=1),
    _t("tail 128-256-32", [50, 128, 256, 32, 1], acts=[1, 2, 1, 0]),
    _t("tail 120-250-30", [50, 120, 250, 30, 1], acts=[3, 1, 2, 3], head=1, extra=True),
    _t("tail 512-64-128", [429, 512, 64, 128, 1], acts=[1, 1, 2, 0], head=1),
    _t("tail 500-60-120", [77, 500, 60, 120, 1], acts=[2, 3, 1, 0]),
    _t("tail 1024-32-256", [20, 1024, 32, 256, 1], acts=[1, 2, 1, 0]),
    _t("tail 1010-20-250", [20, 1010, 20, 250, 1], acts=[1, 1, 3, 2], head=1, extra=True),
    _t("tail 256-128-64 + 1->1", [37, 256, 128, 64, 1, 1], acts=[1, 1, 1, 0, 3]),
    _t("tail 250-120-60 + 1->1", [37, 250, 120, 60, 1, 1], acts=[1, 2, 1, 1, 0], head=1, extra=True),
    _t("tail 512-64-128 + 1->1", [33, 512, 64, 128, 1, 1], acts=[1, 1, 1, 2, 0], head=1),
    # near-misses: (gwa, gwb) = (4, 2), (8, 4), (4, 1) are accepted by mlp_tail_ok and not by mlp_run; last width 2
    _t("near (4,2)", [37, 128, 128, 64, 1], acts=[1, 1, 1, 0], head=1, extra=True),
    _t("near (8,4)", [37, 256, 128, 128, 1], acts=[1, 2, 1, 0]),
    _t("near (4,1)", [37, 128, 128, 32, 1], acts=[1, 1, 3, 0]),
    _t("near last 2", [37, 256, 128, 64, 2], acts=[1, 1, 1, 0]),
    # narrow layers: (T, G, S) = (1,1,1) (2,1,1) (3,2,2) (1,3,3) (3,1,1) (1,3,3); then (2,2,2) (1,2,2) (3,1,1)
    _t("narrow 1", [16, 16, 32, 48, 16, 40, 3]),
    _t("narrow 2", [32, 32, 20, 16, 48, 1], head=1, extra=True),
    _t("narrow K=1024 T=1", [1024, 16, 1], acts=[1, 0]),     # 16 slices of 4 k-groups; the head over S > 1: no fhead
    _t("narrow K=1000 T=3", [1000, 40, 2], acts=[2, 0]),     # 5 slices over 63 k-groups: uneven parts
    _t("fhead G=1", [16, 16, 1], acts=[3, 0]),
    _t("160 KB", [1024, 1024, 512, 256, 128], acts=[1, 2, 1, 0]),
    _t("head no extra", [37, 64, 1], acts=[1, 0], head=1),
    _t("no bias", [37, 64, 5], acts=[2, 1], no_bias=(0, 1), no_alpha=(0,)),
    _t("in_rows", [20, 24, 3], acts=[1, 0], in_rows=True),
    _t("in_rows tail", [45, 256, 128, 64, 1], acts=[1, 1, 1, 0], head=1, extra=True, in_rows=True),
    _t("affine", [37, 64, 5], acts=[2, 0], mode="affine"),
    _t("affine tail", [64, 256, 128, 64, 1], acts=[2, 2, 2, 3], mode="affine"),
    _t("pieces", [20, 40, 1], acts=[2, 3], mode="pieces", x=True),
    _t("pieces no x", [11, 40, 3], acts=[1, 0], mode="pieces", x=False),
    _t("pieces tail", [64, 256, 128, 64, 1], acts=[2, 2, 2, 3], mode="pieces", x=True),
    _t("pieces tail no x", [11, 250, 120, 60, 1], acts=[2, 2, 2, 3], mode="pieces", x=False),
]
for _i, _c in enumerate(TOWER_CASES):
    _c["M"] = _c["M"] or BATCHES[_i % len(BATCHES)]
    _c["seed"] = 500 + _i
TOWER_BY_NAME = {c["name"]: c for c in TOWER_CASES}
PIECE_VOCAB = 9


def _piece_plan(K0, with_x):
    """rs_mlp_affine_pieces_fwd's pieces: (width, input column, sparse?).  with_x: x provides the columns between."""
    return [(6, 2, True), (5, 10, False)] + ([(K0 - 20, 20, True)] if K0 > 20 else []) if with_x else \
        [(6, 0, True), (K0 - 6, 6, False)]


def tower_inputs(c, dt=F64, bad=None):
    """The case's arrays (fp32 values) and its reference in dt: (arrays, ref, flag expected)."""
    rng = np.random.default_rng(c["seed"])
    dims, M = c["dims"], c["M"]
    a = dict(layers=_layers(rng, dims, c["acts"], c.get("no_bias", ()), c.get("no_alpha", ())))
    a["x"] = _nrm(rng, M, dims[0])
    a["extra"] = _nrm(rng, M) if c["extra"] else None
    c0, c1 = (0.5, 0.25) if c["extra"] else (2.0, 1.0)
    a["c0"], a["c1"] = c0, c1
    layers, x = a["layers"], a["x"]
    scale = shift = None
    if c.get("in_rows"):
        # LDS column p reads Keras kernel row in_rows[p]; -1: the column is ignored (a fifth of them)
        K0, Kp = dims[0], rup(dims[0], 16)
        rows = np.full(Kp, -1, np.int32)
        rows[:K0] = rng.permutation(K0)
        rows[:K0][rng.random(K0) < 0.2] = -1
        a["in_rows"] = rows
        W0 = np.where((rows[:K0] >= 0)[:, None], layers[0][0][np.maximum(rows[:K0], 0)], F32(0))
        layers = [(W0,) + layers[0][1:]] + layers[1:]
    if c["mode"] != "plain":
        # BatchNormalization folded as rs_affine_act: scale = gamma / sqrt(var + eps), shift = beta - mean scale
        mean, var = _nrm(rng, dims[0]), rng.random(dims[0]).astype(F32) + F32(0.5)
        gamma, beta = _nrm(rng, dims[0]), _nrm(rng, dims[0]) * F32(0.1)
        scale = (gamma / np.sqrt(var + F32(1e-3))).astype(F32)
        shift = (beta - mean * scale).astype(F32)
        a["bn"], a["scale"], a["shift"] = (mean, var, gamma, beta), scale, shift
    flag = 0
    if c["mode"] == "pieces":
        plan = _piece_plan(dims[0], c["x"])
        a["plan"], a["tables"], a["ids"], a["vals"] = plan, [], [], []
        x = x.copy()
        for pi, (w, col, sparse) in enumerate(plan):
            if sparse:
                table, ids = _nrm(rng, PIECE_VOCAB, w), rng.integers(0, PIECE_VOCAB, M)
                if bad is not None and pi == 0:
                    ids[M - 1 if bad else 0] = PIECE_VOCAB if bad else -1
                    flag = _lib.FLAG_BAD_ID
                ok = (ids >= 0) & (ids < PIECE_VOCAB)
                x[:, col:col + w] = table[np.where(ok, ids, 0)] * ok[:, None]
                a["tables"].append(table), a["ids"].append(ids), a["vals"].append(None)
            else:
                vals = _nrm(rng, M, w)
                x[:, col:col + w] = vals
                a["tables"].append(None), a["ids"].append(None), a["vals"].append(vals)
    ref = ref_tower(x, layers, c["acts"], scale, shift, c["head"], a["extra"], c0, c1, dt)
    return a, ref, flag


def _fm_params(rng, d, kfm):
    return _nrm(rng, 1), _nrm(rng, d) * F32(0.1), _nrm(rng, d, kfm) / F32(np.sqrt(d))


def _ids(rng, B, vocab):
    return np.stack([rng.integers(0, v, B) for v in vocab], 1).astype(np.int64)


def _with_bad(ids, vocab, bad):
    """One out-of-range id: bad = 1: == vocab in the last field of the last sample; 0: -1 in the first of the first."""
    ids = ids.copy()
    if bad == 1:
        ids[-1, -1] = vocab[-1]
    elif bad == 0:
        ids[0, 0] = -1
    return ids, (None if bad is None else (len(ids) - 1 if bad else 0))


def _fm(name, nd, F, k, kfm, dims, acts=None, opts=(0,), logit=True, c=(0.5, 0.5)):
    L = len(dims) - 1
    assert dims[0] == nd + F * k
    return dict(name=name, nd=nd, F=F, k=k, kfm=kfm, dims=list(dims),
                acts=[1] * (L - 1) + [0] if acts is None else acts,
                opts=opts, logit=logit, c0=c[0], c1=c[1])


ALL = (0, 1, 2, 3)
DEEPFM_CASES = [
    _fm("criteo tail", 13, 26, 16, 10, [429, 256, 128, 64, 1], opts=ALL),
    _fm("criteo tail padded", 13, 26, 16, 10, [429, 250, 120, 60, 1], acts=[2, 1, 3, 0], opts=ALL, logit=False),
    _fm("criteo generic tail", 13, 26, 16, 10, [429, 256, 64, 128, 1], opts=ALL),  # Kp[1] = 256, T = 4: gwa 4, no tail
    _fm("criteo no tail", 13, 26, 16, 10, [429, 256, 128, 1], opts=ALL, c=(0.25, 2.0)),
    _fm("Np1>>4 = 7", 13, 26, 16, 10, [429, 256, 112, 1], opts=(0, 2)),
    _fm("first 240", 13, 26, 16, 10, [429, 240, 128, 1], opts=(0, 2)),
    _fm("first 241", 13, 26, 16, 10, [429, 241, 128, 1], opts=(0, 2), acts=[2, 3, 0]),
    _fm("L1", 13, 26, 16, 10, [429, 1], opts=(0, 2)),
    _fm("L2", 13, 26, 16, 10, [429, 256, 1], opts=(0, 2)),
    _fm("nd12", 12, 26, 16, 10, [428, 256, 128, 64, 1], opts=(0, 2, 3)),
    _fm("nd16", 16, 26, 16, 10, [432, 256, 128, 64, 1], opts=(0, 3), logit=False),
    _fm("nd17", 17, 26, 16, 10, [433, 256, 128, 64, 1], opts=(0, 2)),
    _fm("nd1", 1, 26, 16, 10, [417, 256, 128, 64, 1], opts=(0, 2)),
    _fm("nd0", 0, 26, 16, 10, [416, 256, 128, 64, 1], opts=(0, 2)),
    _fm("ptot 1024", 13, 26, 16, 10, [429, 256, 128, 64, 48, 1], opts=(0, 2)),
    _fm("ptot 1056", 13, 26, 16, 10, [429, 256, 128, 64, 64, 1], opts=(0, 2)),
    _fm("kfm1", 13, 26, 16, 1, [429, 256, 128, 64, 1], opts=(0, 3)),
    _fm("kfm15", 13, 26, 16, 15, [429, 256, 128, 64, 1], opts=(0, 2)),
    _fm("120 KB", 13, 26, 16, 10, [429, 768, 112, 1]),
    _fm("F1", 0, 1, 16, 4, [16, 8, 1]),
    _fm("F1 k8", 1, 1, 8, 4, [9, 1]),
    _fm("F9 k8", 3, 9, 8, 6, [75, 32, 1], logit=False),
    _fm("F26 k8", 13, 26, 8, 10, [221, 256, 128, 64, 1], opts=(0, 2)),
    # fewer fields than waves, with dense features: the waves that own the dense k-steps have no field
    _fm("F9 k16", 3, 9, 16, 6, [147, 32, 1]),
    _fm("F15 k8 nd64", 64, 15, 8, 10, [184, 64, 1]),
    _fm("F32 nd64", 64, 32, 8, 10, [320, 64, 1]),
    _fm("F32 nd65", 65, 32, 8, 10, [321, 64, 1]),
    _fm("F32 k16 nd64", 64, 32, 16, 8, [576, 256, 128, 64, 1]),
    _fm("F33", 13, 33, 16, 10, [541, 256, 128, 64, 1]),
    _fm("F33 k8", 0, 33, 8, 10, [264, 40, 1], logit=False),
    _fm("F96 k8", 0, 96, 8, 10, [768, 32, 1]),  # the most fields the 120 KB bound admits (see test_bounds)
]
for _i, _c in enumerate(DEEPFM_CASES):
    _c["B"], _c["seed"] = BATCHES[_i % len(BATCHES)], 900 + _i


def deepfm_inputs(c, dt=F64, bad=None):
    rng = np.random.default_rng(c["seed"])
    nd, F, k, kfm, B = c["nd"], c["F"], c["k"], c["kfm"], c["B"]
    a = dict(vocab=rng.integers(2, 50, F))
    a["table"] = _nrm(rng, int(a["vocab"].sum()), k) * F32(0.5)
    a["dense"] = rng.random((B, nd)).astype(F32)
    a["w0"], a["w1"], a["v"] = _fm_params(rng, c["dims"][0], kfm)
    a["layers"] = _layers(rng, c["dims"], c["acts"])
    a["ids"], a["bad_row"] = _with_bad(_ids(rng, B, a["vocab"]), a["vocab"], bad)
    x = _x_of(a["dense"], a["ids"], a["vocab"], a["table"], dt)
    out, fm = ref_deepfm(x, a["w0"], a["w1"], a["v"], a["layers"], c["acts"], c["c0"], c["c1"], dt)
    a["fm_abs"] = ref_fm(x, a["w0"], a["w1"], a["v"], dt, ab=True)
    return a, out, fm


def _dc(name, nd, F, k, n_cross, dims, acts=None):
    L = len(dims) - 1
    assert dims[0] == nd + F * k
    return dict(name=name, nd=nd, F=F, k=k, n_cross=n_cross, dims=list(dims),
                acts=[1] * (L - 1) + [0] if acts is None else acts)


DCN_CASES = [
    _dc("tail", 13, 26, 16, 3, [429, 256, 128, 64, 1]),
    _dc("tail padded L15", 13, 26, 16, 15, [429, 250, 120, 60, 1], acts=[2, 1, 3, 0]),
    _dc("generic tail", 13, 26, 16, 1, [429, 512, 64, 128, 1]),
    _dc("generic tail padded", 16, 32, 16, 2, [528, 120, 250, 30, 1], acts=[1, 2, 1, 0]),
    _dc("no tail", 13, 26, 16, 1, [429, 64, 32, 1]),
    _dc("L0", 13, 26, 16, 0, [429, 40, 1]),
    _dc("L16 tail dims", 13, 26, 16, 16, [429, 256, 128, 64, 1]),
    _dc("L17", 2, 3, 16, 17, [50, 24, 1]),
    _dc("L31", 13, 26, 16, 31, [429, 40, 1], acts=[3, 0]),
    _dc("k8 L17", 5, 10, 8, 17, [85, 32, 1]),
    _dc("k8 L31", 0, 4, 8, 31, [32, 1]),
    _dc("k4 L0", 3, 7, 4, 0, [31, 16, 1]),
    _dc("k4 L15", 3, 7, 4, 15, [31, 16, 1], acts=[2, 0]),
    _dc("F33 tail dims", 0, 33, 16, 2, [528, 256, 128, 64, 1]),
    _dc("F33 L16", 0, 33, 16, 16, [528, 48, 1]),
    _dc("100 KB", 128, 32, 16, 2, [640, 256, 112, 1]),
    _dc("F1", 1, 1, 16, 1, [17, 8, 1]),
]
for _i, _c in enumerate(DCN_CASES):
    _c["B"], _c["seed"] = BATCHES[_i % len(BATCHES)], 1300 + _i


def dcn_inputs(c, dt=F64, bad=None):
    """The output Dense folded as rs_capi.h asks: cross_prepared over [w_0 .. w_{L-1}, w_o[:d]] (bias row 0), the
    tower's last layer (wf, bf) already the product with w_o[d:]: the reference's output Dense is [w_o[:d] | 1]."""
    rng = np.random.default_rng(c["seed"])
    nd, F, k, L, B = c["nd"], c["F"], c["k"], c["n_cross"], c["B"]
    d = nd + F * k
    a = dict(vocab=rng.integers(2, 50, F))
    a["table"] = _nrm(rng, int(a["vocab"].sum()), k) * F32(0.5)
    a["dense"] = rng.random((B, nd)).astype(F32)
    a["cw"], a["cb"] = _nrm(rng, L, d) * F32(0.05 / np.sqrt(d)), _nrm(rng, L, d) * F32(0.1)
    a["wo"] = _nrm(rng, d) / F32(np.sqrt(d))
    a["layers"] = _layers(rng, c["dims"], c["acts"])
    a["ids"], a["bad_row"] = _with_bad(_ids(rng, B, a["vocab"]), a["vocab"], bad)
    x = _x_of(a["dense"], a["ids"], a["vocab"], a["table"], dt)
    y, alpha = ref_dcn(x, a["cw"], a["cb"], a["layers"], c["acts"], np.concatenate([a["wo"], [F32(1)]]), 0.0, dt)
    a["x"] = x
    return a, y, alpha


def _dn(name, T, k, dims, pooled=True, acts=None):
    return dict(name=name, T=T, k=k, dims=list(dims), pooled=pooled, acts=[2, 2, 2, 3] if acts is None else acts)


DIN_CASES = [
    _dn("k4 T20", 20, 4, [64, 256, 128, 64, 1]),
    _dn("k4 T64 no pieces", 64, 4, [8, 256, 128, 64, 1], pooled=False),
    _dn("k8 T48", 48, 8, [64, 256, 128, 64, 1], pooled=False),
    _dn("k8 T49", 49, 8, [64, 256, 128, 64, 1]),
    _dn("k8 T96", 96, 8, [16, 256, 128, 64, 1]),
    _dn("k8 T97", 97, 8, [64, 256, 128, 64, 1]),
    _dn("k8 T100 no pieces", 100, 8, [16, 256, 128, 64, 1], pooled=False),
    _dn("k8 T112", 112, 8, [64, 250, 120, 60, 1]),
    _dn("k8 T113", 113, 8, [64, 256, 128, 64, 1], pooled=False),
    _dn("k16 T1", 1, 16, [64, 256, 128, 64, 1]),
    _dn("k16 T33 no pieces", 33, 16, [32, 256, 128, 64, 1]),
    _dn("k16 T128", 128, 16, [64, 256, 128, 64, 1], acts=[1, 2, 3, 0]),
]
for _i, _c in enumerate(DIN_CASES):
    _c["B"], _c["seed"] = BATCHES[_i % len(BATCHES)], 1700 + _i
DIN_H, DIN_VOCAB = (80, 40), 50


def din_inputs(c, dt=F64, bad=None):
    """bad: 'hist' / 'cand' / 'piece': one id == vocab there (last sample), or -1 (first sample, bad + '-')."""
    rng = np.random.default_rng(c["seed"])
    T, k, B, dims = c["T"], c["k"], c["B"], c["dims"]
    H1, H2 = DIN_H
    a = dict(table=_nrm(rng, DIN_VOCAB, k) * F32(0.5))
    hist = rng.integers(1, DIN_VOCAB, (B, T))
    hist[rng.random((B, T)) < 0.3] = 0  # padding positions
    hist[0] = 0                          # a fully masked history averages its keys
    if B > 1:
        hist[1] = rng.integers(1, DIN_VOCAB, T)
    cand = rng.integers(0, DIN_VOCAB, B)
    a["att"] = (_nrm(rng, 4 * k, H1) / F32(np.sqrt(4 * k)), _nrm(rng, H1) * F32(0.1), _nrm(rng, T, H1) * F32(0.5),
                _nrm(rng, H1, H2) / F32(np.sqrt(H1)), _nrm(rng, H2) * F32(0.1), _nrm(rng, T, H2) * F32(0.5),
                _nrm(rng, H2) / F32(np.sqrt(H2)), _nrm(rng, 1) * F32(0.1))
    K0 = dims[0]
    mean, var = _nrm(rng, K0), rng.random(K0).astype(F32) + F32(0.5)
    gamma, beta = _nrm(rng, K0), _nrm(rng, K0) * F32(0.1)
    a["scale"] = (gamma / np.sqrt(var + F32(1e-3))).astype(F32)
    a["shift"] = (beta - mean * a["scale"]).astype(F32)
    a["layers"] = _layers(rng, dims, c["acts"])
    # the pieces over columns 2k .. K0-1: a sparse piece of width 6, then dense values
    rest = K0 - 2 * k
    a["plan"] = [] if rest == 0 else [(6, 2 * k, True), (rest - 6, 2 * k + 6, False)]
    a["ptable"], a["pids"] = _nrm(rng, PIECE_VOCAB, 6), rng.integers(0, PIECE_VOCAB, B)
    a["pvals"] = _nrm(rng, B, max(rest - 6, 1))
    row = None
    if bad:
        first = bad.endswith("-")
        row, val = (0, -1) if first else (B - 1, None)
        if bad.startswith("hist"):
            hist[row, T // 2] = DIN_VOCAB if val is None else val
        elif bad.startswith("cand"):
            cand[row] = DIN_VOCAB if val is None else val
        else:
            a["pids"][row] = PIECE_VOCAB if val is None else val
    a["hist"], a["cand"], a["bad_row"] = hist, cand, row
    ok = (a["pids"] >= 0) & (a["pids"] < PIECE_VOCAB)
    other = np.zeros((B, 0), F32) if rest == 0 else \
        np.concatenate([a["ptable"][np.where(ok, a["pids"], 0)] * ok[:, None], a["pvals"]], 1)
    y, pooled = ref_din(hist, cand, a["table"], a["att"], other, a["scale"], a["shift"], a["layers"], c["acts"], dt)
    return a, y, pooled


# --------------------------------------------------------------------------
# A. CPU: the references are the oracle's functions, and a hand-computed tower
# --------------------------------------------------------------------------
def _pin(got, ref, what):
    got, ref = _d(got), _d(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.all(np.abs(got - ref) <= 1e-12 * np.maximum(1.0, np.abs(ref))), \
        f"{what}: off the oracle by {float(np.max(np.abs(got - ref))):.3e}"


def test_tower_by_hand():
    """x = (1, -2); layer 0: W = [[1, 2], [3, 4]], b = (0.5, -0.5), PReLU alpha (0.5, 0.25): z = (1 - 6 + 0.5,
    2 - 8 - 0.5) = (-4.5, -6.5) -> (-2.25, -1.625); layer 1: W = [[2], [-4]], b = 1, linear: -4.5 + 6.5 + 1 = 3;
    head: sigmoid(0.5 * 3 + 0.25 * 2) = sigmoid(2)."""
    layers = [(np.array([[1., 2.], [3., 4.]]), np.array([.5, -.5]), np.array([.5, .25])),
              (np.array([[2.], [-4.]]), np.array([1.]), None)]
    x = np.array([[1., -2.]])
    assert ref_tower(x, layers[:1], [2])[0].tolist() == [-2.25, -1.625]
    assert ref_tower(x, layers, [2, 0])[0, 0] == 3.0
    assert ref_tower(x, layers, [2, 0], head=1, extra=[2.0], c0=0.5, c1=0.25)[0] == 1.0 / (1.0 + np.exp(-2.0))
    # the input affine, ReLU, sigmoid, a missing bias
    assert ref_tower(x, [(np.eye(2), None, None)], [1], np.array([2., 3.]), np.array([1., 1.]))[0].tolist() == [3., 0.]
    assert ref_tower(np.zeros((1, 2)), [(np.eye(2), None, None)], [3])[0].tolist() == [0.5, 0.5]


def test_refs_pinned_tower_and_models():
    rng = np.random.default_rng(11)
    B, nd, k, vocab = 5, 3, 4, np.array([4, 3, 5])
    F, d = len(vocab), 3 + 3 * 4
    tables = [rng.normal(size=(v, k)) for v in vocab]
    table = np.concatenate(tables)
    dense, ids = rng.random((B, nd)), _ids(rng, B, vocab)
    x = _x_of(dense, ids, vocab, table)
    dims = [d, 7, 6, 1]
    W = [rng.normal(size=(a, b)) for a, b in zip(dims[:-1], dims[1:])]
    bs = [rng.normal(size=b) for b in dims[1:]]
    al = [rng.normal(size=b) for b in dims[1:]]
    # the tower, layer by layer, on O.dense; every activation
    for act in range(4):
        h = x
        for l in range(3):
            h = O.dense(h, W[l], bs[l], ACTS[act], al[l])
        _pin(ref_tower(x, list(zip(W, bs, al)), [act] * 3), h, "tower " + ACTS[act])
    mean, var, gamma, beta = rng.normal(size=d), rng.random(d) + 0.5, rng.normal(size=d), rng.normal(size=d)
    scale = gamma / np.sqrt(var + 1e-3)
    _pin(ref_tower(x, [(W[0], bs[0], None)], [1], scale, beta - mean * scale),
         O.dense(O.batchnorm_inference(x, mean, var, gamma, beta, 1e-3), W[0], bs[0], "relu"), "affine tower")
    # DeepFM
    kfm = 3
    w0, w1, v = rng.normal(size=1), rng.normal(size=(d, 1)), rng.normal(size=(d, kfm))
    p = {"tables": tables, "w0": w0, "w1": w1, "v": v, "dnn_hidden": list(zip(W[:2], bs[:2])), "dnn_out": (W[2], bs[2])}
    ref, ref_fm_, _ = O.deepfm(None, p, inputs=(dense, ids))
    layers = [(W[0], bs[0], None), (W[1], bs[1], None), (W[2], bs[2], None)]
    out, fm = ref_deepfm(x, w0, w1, v, layers, [1, 1, 0], 0.5, 0.5)
    _pin(fm, ref_fm_[:, 0], "FM logit")
    _pin(out, ref[:, 0], "DeepFM")
    assert np.all(ref_fm(x, w0, w1, v, ab=True) >= np.abs(fm))
    # DCN: the unfolded output Dense, and the folded form the kernel is given
    L = 3
    cw, cb = rng.normal(size=(L, d)) / np.sqrt(d), rng.normal(size=(L, d))
    Wl, bl = rng.normal(size=(6, 4)), rng.normal(size=4)
    ok, ob = rng.normal(size=(d + 4, 1)), rng.normal(size=1)
    p = {"tables": tables, "cross_w": list(cw), "cross_b": list(cb), "dnn_hidden": list(zip(W[:2], bs[:2])),
         "dnn_out": (Wl, bl), "out_kernel": ok, "out_bias": ob}
    ref, cross = O.dcn(None, p, inputs=(dense, ids))
    hid = [(W[0], bs[0], None), (W[1], bs[1], None)]
    y, alpha = ref_dcn(x, cw, cb, hid + [(Wl, bl, None)], [1, 1, 0], ok, ob)
    _pin(y, ref[:, 0], "DCN")
    _pin(ref_cross(x, cw, cb)[0], cross, "CrossNet")
    _pin(ref_cross(x, cw, cb)[0], alpha[:, None] * x + cb.sum(0), "x_L = alpha_L x0 + beta_L")
    fold = (Wl @ ok[d:], bl @ ok[d:] + ob, None)
    _pin(ref_dcn(x, cw, cb, hid + [fold], [1, 1, 0], np.concatenate([ok[:d, 0], [1.0]]), 0.0)[0], ref[:, 0],
         "DCN with the last layer folded")
    _pin(ref_dcn(x, cw[:0], cb[:0], hid + [fold], [1, 1, 0], np.concatenate([ok[:d, 0], [1.0]]), 0.0)[0],
         O.dcn(None, dict(p, cross_w=[], cross_b=[]), inputs=(dense, ids))[0][:, 0], "DCN without cross layers")


def test_ref_pinned_din():
    rng = np.random.default_rng(12)
    B, T, k, V, H1, H2 = 4, 5, 4, 9, 6, 5
    table = rng.normal(size=(V, k))
    hist = rng.integers(0, V, (B, T))
    hist[0] = 0
    cand = rng.integers(0, V, B)
    att = (rng.normal(size=(4 * k, H1)), rng.normal(size=H1), rng.normal(size=(T, H1)), rng.normal(size=(H1, H2)),
           rng.normal(size=H2), rng.normal(size=(T, H2)), rng.normal(size=(H2, 1)), rng.normal(size=1))
    gt, gender = rng.normal(size=(3, 2)), rng.integers(0, 3, B)
    age = rng.random(B)
    K0 = 2 * k + 3
    bn = (rng.normal(size=K0), rng.normal(size=K0), rng.normal(size=K0), rng.random(K0) + 0.5, 1e-3)
    dnn = [(rng.normal(size=(K0, 7)), rng.normal(size=7), rng.normal(size=7)),
           (rng.normal(size=(7, 6)), rng.normal(size=6), rng.normal(size=6))]
    out = (rng.normal(size=(6, 1)), rng.normal(size=1))
    p = {"sparse_tables": {"gender": gt}, "seq_tables": {"hist": table}, "bn": bn, "dnn": dnn, "out": out,
         "att": {"prelu": [(att[0], att[1], att[2]), (att[3], att[4], att[5])], "out": (att[6], att[7])}}
    ref, pooled_ref = O.din({"age": age, "gender": gender, "movie_id": cand, "hist": hist}, p, ["age"],
                            ["gender", "hist"], ["hist"])
    g, bt, mu, var, eps = bn
    scale = g / np.sqrt(var + eps)
    other = np.concatenate([gt[gender], age.astype(np.float32).astype(F64)[:, None]], 1)
    y, pooled = ref_din(hist, cand, table, att, other, scale, bt - mu * scale,
                        [(w, b, a) for w, b, a in dnn] + [(out[0], out[1], None)], [2, 2, 3])
    _pin(pooled, pooled_ref, "DIN attention")
    _pin(y, ref[:, 0], "DIN")
    _pin(pooled[0], table[0], "a fully masked history averages its (equal) keys")


# --------------------------------------------------------------------------
# A. CPU: every launch line is named by a case
# --------------------------------------------------------------------------
def _case_branches():
    """Every GPU case as the set of kernels it launches: {launcher: {kernel: [case names]}}."""
    seen = {"mlp_run": {}, "launch_deepfm": {}, "dcn_run": {}, "launch_din_tower": {}}
    for c in TOWER_CASES:
        seen["mlp_run"].setdefault(tower_branch(c["dims"], c["mode"] == "pieces")[0], []).append(c["name"])
    for c in DEEPFM_CASES:
        for hm in (True, False):
            for opt in c["opts"] if hm else (0,):
                seen["launch_deepfm"].setdefault(deepfm_branch(c["nd"], c["F"], c["k"], c["kfm"], c["dims"], hm, opt),
                                                 []).append((c["name"], hm, opt))
    for c in DCN_CASES:
        for hm in (True, False):
            for opt in (0, 1):
                seen["dcn_run"].setdefault(dcn_branch(c["nd"], c["F"], c["k"], c["n_cross"], c["dims"], hm, opt),
                                           []).append((c["name"], hm, opt))
    for c in DIN_CASES:
        seen["launch_din_tower"].setdefault(din_branch(c["T"], c["k"], *DIN_H, c["dims"])[0], []).append(c["name"])
    return seen


def _launch_lines(path, func):
    """The kernels named by launch_lds<...> in the body of `func` of csrc/<path>, with KV / KS / KIND / MLP_NW
    expanded as the callers instantiate them."""
    src = open(os.path.join(CSRC, path)).read()
    start = src.index(func)
    body = src[start:src.index("\n}\n", start)]
    names = re.findall(r"launch_lds<(\w+<[^;()]*?>)>\(", body)
    out = set()
    for n in names:
        n = n.replace("KIND, ", "").replace(", KIND", "").replace("MLP_NW", "16").replace(" ", "")
        if "KV" in n:
            out |= {n.replace("KV", "2"), n.replace("KV", "4")}
        elif "KS" in n:
            out |= {n.replace("KS", s) for s in ("1", "2", "4")}
        else:
            out.add(n)
    return out


def test_every_launch_line_is_named_by_a_case():
    """The instantiations (the id kind left out: every case runs int32, int64 and float32 ids):
    mlp.hip:219-224 mlp_run: mlp_tower_pc<16,true>, mlp_tower_pc<16>, mlp_tower<16,true>, mlp_tower<16>;
    deepfm.hip:609-626 launch_deepfm<KV>: deepfm_all<27,4,8,2>, deepfm_all<27,3,8,2>, deepfm_all<27,3>,
    deepfm_ws<27,8,2>, deepfm_ws<27>, deepfm_fused_ka<2>, deepfm_fused_ka<4>, deepfm_fused<2>, deepfm_fused<4>;
    cross.hip:856-867 dcn_run: dcn_fused_ka<1,true,true>, dcn_fused_ka<1,true>, dcn_fused_ka<1,false,true>,
    dcn_fused_ka<1>, dcn_fused_ka<2>, dcn_fused<1>, dcn_fused<2>;
    din.hip:1005-1006 launch_din_tower<KS>: din_fused_tower<2,5,3,7> (KS = 2 alone reaches NTT = 7's form: the
    branch tests KS), din_fused_tower<1,5,3>, din_fused_tower<2,5,3>, din_fused_tower<4,5,3>.
    The lists are read from the sources, so a launch line added later fails here until a case names it."""
    want = {"mlp_run": _launch_lines("mlp.hip", "static int mlp_run("),
            "launch_deepfm": _launch_lines("deepfm.hip", "static void launch_deepfm("),
            "dcn_run": _launch_lines("cross.hip", "static int dcn_run("),
            "launch_din_tower": _launch_lines("din.hip", "static void launch_din_tower(")}
    want["launch_din_tower"] -= {"din_fused_tower<1,5,3,7>", "din_fused_tower<4,5,3,7>"}  # KS == 2 && NTT == 7
    assert [len(want[k]) for k in ("mlp_run", "launch_deepfm", "dcn_run", "launch_din_tower")] == [4, 9, 7, 4], want
    seen = _case_branches()
    for launcher, kernels in want.items():
        assert kernels == set(seen[launcher]), (launcher, kernels ^ set(seen[launcher]))
    # ... and the branches inside the tower's body
    feats = {}
    for c in TOWER_CASES:
        kern, f = tower_branch(c["dims"], c["mode"] == "pieces")
        for x in f:
            feats.setdefault((kern.split("<")[0].replace("_pc", "") + kern[kern.index("<"):], x), []).append(c["name"])
    for key in [("mlp_tower<16,true>", "layer0_tiles"), ("mlp_tower<16,true>", "tower_tile(0,1)"),
                ("mlp_tower<16,true>", "tail<8,2,8,4>"), ("mlp_tower<16,true>", "tail<8,2>"),
                ("mlp_tower<16,true>", "extra 1->1"), ("mlp_tower<16>", "fhead"), ("mlp_tower<16>", "S>1"),
                ("mlp_tower<16>", "S=1"), ("mlp_tower<16>", "T>16 (a wave's second item)")]:
        assert feats.get(key), key
    # the near-misses are near: mlp_tail_ok accepts them, mlp_run (gwa == 8 && gwb == 2) does not
    for name, gw in (("near (4,2)", (4, 2)), ("near (8,4)", (8, 4)), ("near (4,1)", (4, 1)), ("near last 2", None)):
        c = TOWER_BY_NAME[name]
        assert mlp_tail_ok(mlp_geom(c["dims"])) == gw and tower_branch(c["dims"])[0] == "mlp_tower<16>", name
    # the generic tail with and without the trailing layer, on a first layer of 256 units and on another
    tails = {tuple(tower_branch(c["dims"])[1]) for c in TOWER_CASES if tower_branch(c["dims"])[0].endswith("true>")}
    assert {("layer0_tiles", "tail<8,2,8,4>"), ("layer0_tiles", "tail<8,2,8,4>", "extra 1->1"),
            ("tower_tile(0,1)", "tail<8,2>"), ("tower_tile(0,1)", "tail<8,2>", "extra 1->1")} <= tails
    # narrow layers: 1, 2 and 3 output tiles with 1 and 2 k-groups (fewer k-groups than slices), and S < G
    tgs = {t for c in TOWER_CASES if not _tail82(mlp_geom(c["dims"])) for t in tower_features(mlp_geom(c["dims"]))[1]}
    assert {(1, 1, 1), (2, 1, 1), (3, 1, 1), (1, 2, 2), (2, 2, 2), (3, 2, 2), (1, 3, 3), (1, 64, 16), (3, 63, 5)} <= tgs
    # DIN: both LDS layouts, and NTT = 7 beside 6 and 8
    lay = {din_branch(c["T"], c["k"], *DIN_H, c["dims"]) for c in DIN_CASES}
    assert {k for k, _ in lay} == want["launch_din_tower"] and {t for _, t in lay} == {"tbase=0", "tbase=total"}
    by = {c["name"]: din_branch(c["T"], c["k"], *DIN_H, c["dims"]) for c in DIN_CASES}
    assert by["k8 T48"][1] == "tbase=total" and by["k8 T49"][1] == "tbase=0"
    assert [by[n][0][-3:] for n in ("k8 T96", "k8 T97", "k8 T112", "k8 T113")] == [",3>", ",7>", ",7>", ",3>"]


def test_deepfm_and_dcn_cases_take_the_branches_their_names_say():
    """Both sides of every edge of deepfm_ws_ok / deepfm_all_ok and of the ka / generic choice, and dcn_run's six
    conditions under both RS_OPT_CROSS_KERNEL values: (case, entry, option) -> kernel."""
    fm = {c["name"]: c for c in DEEPFM_CASES}
    br = lambda n, hm, opt: deepfm_branch(fm[n]["nd"], fm[n]["F"], fm[n]["k"], fm[n]["kfm"], fm[n]["dims"], hm, opt)
    assert [br("criteo tail", True, o) for o in ALL] == ["deepfm_ws<27,8,2>", "deepfm_fused_ka<4>",
                                                         "deepfm_all<27,3,8,2>", "deepfm_all<27,4,8,2>"]
    assert [br("criteo tail padded", True, o) for o in ALL] == [br("criteo tail", True, o) for o in ALL]
    assert [br("criteo generic tail", True, o) for o in ALL] == ["deepfm_fused_ka<4>"] * 2 + ["deepfm_all<27,3>"] * 2
    assert [br("criteo no tail", True, o) for o in ALL] == \
        ["deepfm_ws<27>", "deepfm_fused_ka<4>"] + ["deepfm_all<27,3>"] * 2
    assert br("criteo tail", False, 0) == "deepfm_fused<4>"
    assert (br("Np1>>4 = 7", True, 0), br("Np1>>4 = 7", True, 2)) == ("deepfm_fused_ka<4>", "deepfm_all<27,3>")
    assert (br("first 240", True, 0), br("first 240", True, 2)) == ("deepfm_fused_ka<4>",) * 2
    assert (br("first 241", True, 0), br("first 241", True, 2)) == ("deepfm_ws<27>", "deepfm_all<27,3>")
    assert (br("L1", True, 0), br("L1", True, 2)) == ("deepfm_fused_ka<4>",) * 2
    assert (br("L2", True, 0), br("L2", True, 2)) == ("deepfm_fused_ka<4>", "deepfm_all<27,3>")
    assert [br("nd12", True, o) for o in (0, 2, 3)] == \
        ["deepfm_fused_ka<4>", "deepfm_all<27,3,8,2>", "deepfm_all<27,4,8,2>"]
    assert [br("nd16", True, o) for o in (0, 3)] == ["deepfm_ws<27,8,2>", "deepfm_all<27,4,8,2>"]
    assert [br("nd17", True, o) for o in (0, 2)] == ["deepfm_fused_ka<4>"] * 2
    assert [br("nd1", True, o) for o in (0, 2)] == ["deepfm_fused_ka<4>", "deepfm_all<27,3,8,2>"]
    assert [br("nd0", True, o) for o in (0, 2)] == ["deepfm_fused_ka<4>"] * 2
    assert [br("ptot 1024", True, o) for o in (0, 2)] == ["deepfm_ws<27>", "deepfm_all<27,3>"]
    assert [br("ptot 1056", True, o) for o in (0, 2)] == ["deepfm_ws<27>", "deepfm_fused_ka<4>"]
    assert (mlp_geom(fm["ptot 1024"]["dims"])["ptot"], mlp_geom(fm["ptot 1056"]["dims"])["ptot"]) == (1024, 1056)
    assert br("120 KB", True, 0) == "deepfm_fused_ka<4>" and br("F26 k8", True, 2) == "deepfm_fused_ka<2>"
    assert (br("F32 nd64", True, 0), br("F32 nd65", True, 0)) == ("deepfm_fused_ka<2>", "deepfm_fused<2>")
    assert (br("F32 k16 nd64", True, 0), br("F33", True, 0), br("F33 k8", True, 0)) == \
        ("deepfm_fused_ka<4>", "deepfm_fused<4>", "deepfm_fused<2>")
    assert (br("F1", True, 0), br("F1 k8", True, 0), br("F96 k8", True, 0)) == \
        ("deepfm_fused_ka<4>", "deepfm_fused_ka<2>", "deepfm_fused<2>")
    assert (br("F9 k8", True, 0), br("F9 k16", True, 0), br("F15 k8 nd64", True, 0)) == \
        ("deepfm_fused_ka<2>", "deepfm_fused_ka<4>", "deepfm_fused_ka<2>")
    dc = {c["name"]: c for c in DCN_CASES}
    db = lambda n, hm, opt: dcn_branch(dc[n]["nd"], dc[n]["F"], dc[n]["k"], dc[n]["n_cross"], dc[n]["dims"], hm, opt)
    for n in ("tail", "tail padded L15", "generic tail", "generic tail padded"):
        assert (db(n, True, 0), db(n, True, 1), db(n, False, 0)) == \
            ("dcn_fused_ka<1,true,true>", "dcn_fused_ka<1,true>", "dcn_fused<1>"), n
    for n in ("no tail", "L0", "100 KB", "F1"):
        assert (db(n, True, 0), db(n, True, 1), db(n, False, 1)) == \
            ("dcn_fused_ka<1,false,true>", "dcn_fused_ka<1>", "dcn_fused<1>"), n
    for n in ("L16 tail dims", "L17", "L31"):
        assert (db(n, True, 0), db(n, True, 1), db(n, False, 0)) == ("dcn_fused_ka<2>",) * 2 + ("dcn_fused<2>",), n
    for n, nt in (("k8 L17", 2), ("k8 L31", 2), ("k4 L0", 1), ("k4 L15", 1), ("F33 tail dims", 1), ("F33 L16", 2)):
        assert not kernarg_meta(True, dc[n]["F"], dc[n]["k"])  # no metadata: the _hm entry runs the plain kernel
        assert {db(n, hm, o) for hm in (True, False) for o in (0, 1)} == {f"dcn_fused<{nt}>"}, n


# --------------------------------------------------------------------------
# A. CPU: the restated predicates are the library's, on both sides of every bound
# --------------------------------------------------------------------------
def _ci(v):
    return (C.c_int * len(v))(*v)


def test_supported_predicates_match_the_library():
    lib = _lib.lib()
    towers = [[w, 5] for w in (1, 16, 1024, 1025, 0)] + [[5, w] for w in (1, 1024, 1025, 0)] + \
        [[8] * n for n in (1, 2, 9, 10)] + \
        [[1024, 1024, 512, 256, n] for n in (112, 128, 129, 144)] + [[1024, 1024, 512, n, 128] for n in (256, 257)] + \
        [[960, 960, 1024], [961, 64, 64, 64, 64, 64, 64, 64, 64], [1024] * 9, [1024] * 3, [1024, 1024, 1024, 1]]
    for dims in towers:
        g = mlp_geom(dims)
        assert lib.rs_mlp_prepared_size(len(dims) - 1, _ci(dims)) == (g["total"] if g else -1), dims
    for c in TOWER_CASES:
        assert lib.rs_mlp_prepared_size(len(c["dims"]) - 1, _ci(c["dims"])) == mlp_geom(c["dims"])["total"] > 0
    n = 0
    for nd in (-1, 0, 1, 13, 64, 65):
        for F in (0, 1, 26, 32, 33, 96, 128, 129):
            for k in (4, 8, 12, 16, 32):
                for kfm in (0, 1, 15, 16):
                    d = nd + F * k
                    for dims in ([d, 1], [d, 256, 128, 64, 1], [d + 1, 8, 1], [d, 8, 2], [d, 768, 112, 1],
                                 [d, 768, 128, 1], [d, 769, 1], [d, 704, 576, 1], [d, 704, 592, 1]):
                        assert lib.rs_deepfm_fused_ok(nd, F, k, kfm, len(dims) - 1, _ci(dims)) == \
                            int(deepfm_supported(nd, F, k, kfm, dims)), (nd, F, k, kfm, dims)
                        n += deepfm_supported(nd, F, k, kfm, dims)
    assert n > 100
    n = 0
    for nd in (-1, 0, 13, 128):
        for F in (0, 1, 32, 33, 128, 129):
            for k in (0, 2, 4, 6, 8, 16, 20):
                for L in (-1, 0, 16, 31, 32):
                    d = nd + F * k
                    for dims in ([d, 1], [d, 256, 128, 64, 1], [d + 1, 8, 1], [d, 8, 2], [d, 256, 112, 1],
                                 [d, 256, 128, 1], [d, 640, 1], [d, 641, 1], [d, 576, 176, 1], [d, 576, 192, 1]):
                        assert lib.rs_dcn_fused_ok(nd, F, k, L, len(dims) - 1, _ci(dims)) == \
                            int(dcn_supported(nd, F, k, L, dims)), (nd, F, k, L, dims)
                        n += dcn_supported(nd, F, k, L, dims)
    assert n > 100
    n = 0
    for T in (0, 1, 48, 49, 112, 113, 128, 129, 1024, 1025):
        for k in (4, 8, 12, 16, 32):
            for H1, H2 in ((80, 40), (64, 40), (65, 33), (81, 40), (80, 32), (80, 48), (80, 49), (128, 64), (129, 40)):
                for dims in ([64, 256, 128, 64, 1], [2 * k, 256, 128, 64, 1], [2 * k - 1, 256, 128, 64, 1],
                             [65, 256, 128, 64, 1], [64, 241, 113, 49, 1], [64, 240, 128, 64, 1], [64, 256, 128, 1],
                             [64, 256, 128, 64, 2], [64, 256, 128, 64, 1, 1], [64, 256, 128, 128, 1]):
                    assert lib.rs_din_forward_ids_supported(T, k, H1, H2, len(dims) - 1, _ci(dims)) == \
                        int(din_tower(T, k, H1, H2, dims) is not None), (T, k, H1, H2, dims)
                    n += din_tower(T, k, H1, H2, dims) is not None
    assert n > 50
    for c in DEEPFM_CASES:
        assert deepfm_supported(c["nd"], c["F"], c["k"], c["kfm"], c["dims"]), c["name"]
    for c in DCN_CASES:
        assert dcn_supported(c["nd"], c["F"], c["k"], c["n_cross"], c["dims"]), c["name"]
    for c in DIN_CASES:
        assert din_tower(c["T"], c["k"], *DIN_H, c["dims"]), c["name"]


def test_bounds_derived_and_neighbours_refused():
    """The tower's LDS is (32 rs + 16 * 256 + ptot) * 4 B, rs = roundup(widest, 64) + 8, ptot = 2 sum Np.
    rs_mlp_*: <= 160 KB = 40,960 floats.  At a widest layer of 1024 (rs 1032: 33,024 + 4,096) ptot may be 3,840:
    sum Np = 1,920 = 1024 + 512 + 256 + 128: dims [1024, 1024, 512, 256, 128] sits on the bound and one more
    16-unit tile anywhere is refused.  The kernels' static LDS is 0, so the launch asks for exactly 160 KB.
    rs_deepfm_fwd: <= 120 KB = 30,720 floats.  rs = 776 (widest 768) leaves ptot <= 1,792: [429, 768, 112, 1] sits
    on it (768 + 112 + 16 = 896); rs = 840 would leave 30,720 - 26,880 - 4,096 < 0: no layer, and no input, wider
    than 768, so at most 96 fields of k = 8 — the 128 fields rs_capi.h names can never be accepted.  Static LDS of
    deepfm_fused: cs 17,408 + qs 1,024 + fmlog 64 + the id tile 16,384 + 2,048 = 36,928 B; 159,808 <= 163,840.
    rs_dcn_fwd: <= 100 KB = 25,600 floats: rs = 648 (widest 640) leaves ptot <= 768: [640, 256, 112, 1]; static
    LDS of dcn_fused<2>: cs 33,792 + xlog 64 + ids 16,384 + meta 2,048 = 52,288 B; 154,688 <= 163,840."""
    lib = _lib.lib()
    on = [1024, 1024, 512, 256, 128]
    assert mlp_geom(on)["lds"] == 160 * 1024
    c5 = _ci([0] * 5)
    hoff, hvoc = (C.c_int64 * 128)(), (C.c_int64 * 128)()  # the _hm entries read their host metadata before any check
    for i in range(1, 5):
        over = list(on)
        over[i] += 16 if on[i] < 1024 else 0
        if over != on:
            assert mlp_geom(over) is None and lib.rs_mlp_prepared_size(4, _ci(over)) == -1
            _refused(lib.rs_mlp_prepare(4, _ci(over), _p(1), None, None, None, _p(2), None), b"rs_mlp_prepare",
                     b"widths 1..1024")
            _refused(lib.rs_mlp_fwd(_p(1), 1024, 4, _ci(over), c5, _p(2), _p(3), over[-1], 0, None, 1.0, 1.0, 4, None),
                     b"rs_mlp_fwd", b"widths 1..1024")
    assert lib.rs_last_error_string() and lib.rs_mlp_prepared_size(4, _ci([1024, 1024, 512, 256, 129])) == -1
    assert b"160 KB" in lib.rs_last_error_string()
    _refused(lib.rs_mlp_affine_pieces_fwd(None, 0, _p(1), _p(2), 2, _ci([65, 8, 1]), c5, _p(3), _p(4), 1, 0, None,
                                          1.0, 1.0, 4, 1, _ci([65]), _ci([0]), _ci([-1]), (C.c_void_p * 1)(0x1000),
                                          (C.c_int64 * 1)(65), None, None, _p(5), None),
             b"rs_mlp_affine_pieces_fwd", b"at most 64 input columns")
    fm_on, fm_over = [429, 768, 112, 1], [429, 768, 128, 1]
    assert mlp_geom(fm_on)["lds"] == 120 * 1024 and mlp_geom(fm_over)["lds"] == 120 * 1024 + 128
    assert deepfm_supported(13, 26, 16, 10, fm_on) and not deepfm_supported(13, 26, 16, 10, fm_over)
    assert lib.rs_deepfm_fused_ok(13, 26, 16, 10, 3, _ci(fm_on)) == 1
    assert lib.rs_deepfm_fused_ok(13, 26, 16, 10, 3, _ci(fm_over)) == 0
    assert lib.rs_deepfm_fused_ok(13, 26, 16, 10, 2, _ci([429, 784, 1])) == 0  # rs = 840
    fmcall = lambda entry, hm, nd, F, k, dims: getattr(lib, entry)(
        _p(1), 0, F, _p(2), nd, nd, _p(3), _p(4), _p(5), *hm, F, k, _p(6), _p(7), 10, len(dims) - 1, _ci(dims), c5,
        _p(8), 0.5, 0.5, _p(9), None, 4, None, None)
    for entry, hm in (("rs_deepfm_fwd", ()), ("rs_deepfm_fwd_hm", (hoff, hvoc))):
        _refused(fmcall(entry, hm, 13, 26, 16, fm_over), b"rs_deepfm_fwd", b"unsupported shape")
        # d = F k <= 768: 96 fields of k = 8 are the most; 97 and the 128 of the header are refused
        _refused(fmcall(entry, hm, 0, 97, 8, [776, 8, 1]), b"rs_deepfm_fwd", b"unsupported shape")
        _refused(fmcall(entry, hm, 0, 128, 8, [1024, 8, 1]), b"rs_deepfm_fwd", b"unsupported shape")
    assert deepfm_supported(0, 96, 8, 10, [768, 32, 1]) and not deepfm_supported(0, 97, 8, 10, [776, 32, 1])
    dc_on, dc_over = [640, 256, 112, 1], [640, 256, 128, 1]
    assert mlp_geom(dc_on)["lds"] == 100 * 1024 and mlp_geom(dc_over)["lds"] == 100 * 1024 + 128
    assert lib.rs_dcn_fused_ok(128, 32, 16, 2, 3, _ci(dc_on)) == 1
    assert lib.rs_dcn_fused_ok(128, 32, 16, 2, 3, _ci(dc_over)) == 0
    assert lib.rs_dcn_fused_ok(0, 41, 16, 2, 2, _ci([656, 8, 1])) == 0  # rs = 712
    dccall = lambda entry, hm, dims, n_cross=2: getattr(lib, entry)(
        _p(1), 0, 32, _p(2), 128, 128, _p(3), _p(4), _p(5), *hm, 32, 16, n_cross, _p(6), len(dims) - 1, _ci(dims), c5,
        _p(7), _p(8), 4, None, None)
    for entry, hm in (("rs_dcn_fwd", ()), ("rs_dcn_fwd_hm", (hoff, hvoc))):
        _refused(dccall(entry, hm, dc_over), b"rs_dcn_fwd", b"unsupported shape")
        _refused(dccall(entry, hm, dc_on, 32), b"rs_dcn_fwd", b"unsupported shape")
    # the static + dynamic LDS of the widest accepted launch of each family stays within the 160 KB of a workgroup
    assert 17408 + 1024 + 64 + 16384 + 2048 + mlp_geom(fm_on)["lds"] <= 160 * 1024
    assert 33792 + 64 + 16384 + 2048 + mlp_geom(dc_on)["lds"] <= 160 * 1024
    assert max(din_tower(T, k, 80, 40, [64, 256, 128, 64, 1])[1] for T in (1, 48, 49, 128) for k in (4, 8, 16)) + \
        DIN_STATIC <= 160 * 1024
    # DIN: a tower that is not the 256 -> 128 -> 64 -> 1 shape, or wider than 64 columns, keeps the two launches
    din = lambda T, k, dims: lib.rs_din_forward_ids(
        _p(1), 0, T, _p(2), 1, T, k, _p(3), 50, 80, 40, _p(4), None, 0, _p(5), _p(6), len(dims) - 1, _ci(dims), c5,
        _p(7), _p(8), 1, 0, None, None, None, None, None, None, None, 4, _p(9), None)
    _refused(din(129, 8, [16, 256, 128, 64, 1]), b"rs_din_forward_ids", b"not supported by the fused launch")
    _refused(din(100, 8, [65, 256, 128, 64, 1]), b"rs_din_forward_ids", b"not supported by the fused launch")
    _refused(din(100, 8, [16, 240, 128, 64, 1]), b"rs_din_forward_ids", b"not supported by the fused launch")
    _refused(din(100, 12, [24, 256, 128, 64, 1]), b"rs_din_forward_ids", b"k in {4,8,16}")


# --------------------------------------------------------------------------
# A. CPU: every GPU case is well conditioned: float32 numpy within RTOL / 4
# --------------------------------------------------------------------------
def _cond_scaled(lo, ref, what):
    assert_scaled_close(np.asarray(lo, F64), _d(ref), RTOL / 4, "float32 restatement of " + what)


def _cond_rel(lo, ref, what):
    assert_rel_close(np.asarray(lo, F64), _d(ref), RTOL / 4, "float32 restatement of " + what)


@pytest.mark.parametrize("c", TOWER_CASES, ids=lambda c: c["name"])
def test_tower_cases_conditioned(c):
    for bad in (None, 0, 1) if c["mode"] == "pieces" else (None,):
        ref, lo = tower_inputs(c, F64, bad)[1], tower_inputs(c, F32, bad)[1]
        assert lo.dtype == F32 and np.isfinite(ref).all()
        (_cond_rel if c["head"] else _cond_scaled)(lo, ref, "tower " + c["name"])


@pytest.mark.parametrize("c", DEEPFM_CASES, ids=lambda c: c["name"])
def test_deepfm_cases_conditioned(c):
    for bad in (None, 0, 1):
        (a, out, fm), (_, out32, fm32) = deepfm_inputs(c, F64, bad), deepfm_inputs(c, F32, bad)
        assert out32.dtype == F32 and fm32.dtype == F32
        _cond_rel(out32, out, "DeepFM " + c["name"])
        assert np.all(np.abs(_d(fm32) - fm) <= SUM_TOL / 4 * a["fm_abs"]), "float32 FM logit of " + c["name"]


@pytest.mark.parametrize("c", DCN_CASES, ids=lambda c: c["name"])
def test_dcn_cases_conditioned(c):
    for bad in (None, 0, 1):
        (_, y, alpha), (_, y32, _) = dcn_inputs(c, F64, bad), dcn_inputs(c, F32, bad)
        assert np.abs(alpha).max() < 10.0 and y32.dtype == F32
        _cond_rel(y32, y, "DCN " + c["name"])


@pytest.mark.parametrize("c", DIN_CASES, ids=lambda c: c["name"])
def test_din_cases_conditioned(c):
    for bad in (None, "hist", "hist-", "cand", "cand-", "piece", "piece-"):
        (_, y, pooled), (_, y32, pooled32) = din_inputs(c, F64, bad), din_inputs(c, F32, bad)
        assert y32.dtype == F32 and pooled32.dtype == F32
        (_cond_rel if c["acts"][-1] == 3 else _cond_scaled)(y32, y, "DIN " + c["name"])
        _cond_scaled(pooled32, pooled, "DIN pooled " + c["name"])


# --------------------------------------------------------------------------
# B. GPU
# --------------------------------------------------------------------------
WORST = {}  # entry point -> worst error under its comparison


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    yield
    for k in sorted(WORST):
        print(f"\nworst {k}: {WORST[k]:.3e}", end="")


def _host(got, ref):
    return np.asarray(_get(got) if hasattr(got, "detach") else got, F64).reshape(np.shape(ref)), _d(ref)


def _close(kernel, got, ref, what):
    """Raw tower outputs and logits: assert_scaled_close at 1e-5."""
    got, ref = _host(got, ref)
    if ref.size and np.any(ref != 0):
        scale = np.maximum(np.abs(ref), float(np.sqrt(np.mean(ref ** 2))))
        key = kernel + " (scaled)"
        WORST[key] = max(WORST.get(key, 0.0), float(np.nanmax(np.abs(got - ref) / scale)))
    assert_scaled_close(got, ref, RTOL, f"{kernel} {what}")


def _rel(kernel, got, ref, what):
    """Post-sigmoid outputs: assert_rel_close at 1e-5."""
    got, ref = _host(got, ref)
    key = kernel + " (post-sigmoid, relative)"
    WORST[key] = max(WORST.get(key, 0.0), float(np.nanmax(np.abs(got - ref) / np.abs(ref))))
    assert_rel_close(got, ref, RTOL, f"{kernel} {what}")


def _sum_close(kernel, got, ref, absum, what):
    """|got - ref| <= SUM_TOL * sum |terms|: the FM logit (see the module docstring)."""
    got, ref = _host(got, ref)
    ratio = np.abs(got - ref) / _d(absum).reshape(ref.shape)
    key = kernel + " (error / sum |terms|)"
    WORST[key] = max(WORST.get(key, 0.0), float(np.nanmax(ratio)))
    assert np.all(ratio <= SUM_TOL), f"{kernel} {what}: worst {float(np.nanmax(ratio)):.3e} of sum |terms|"


class _option:
    """rs_set_option for a block, the previous value restored in its finally."""

    def __init__(self, option, value):
        self.option, self.value = option, value

    def __enter__(self):
        self.prev = _lib.set_option(self.option, self.value)

    def __exit__(self, *exc):
        _lib.set_option(self.option, self.prev)


def _nan(n):
    return torch.full((max(int(n), 1),), float("nan"), dtype=torch.float32, device="cuda")


def _flag():
    return torch.zeros(1, dtype=torch.int32, device="cuda")


def _pn(t):
    return None if t is None else t.data_ptr()


def _ids_dev(ids, dtype, frac=lambda a: a >= 0):
    """[B, F] ids with row stride F + 2; float ids carry a fraction (Keras truncates them)."""
    a = np.asarray(ids, np.float64)
    if dtype is np.float32:
        a = a + 0.25 * frac(a)
    return _rows(a, 2, np.nan if dtype is np.float32 else 7, dtype)


def _meta(vocab):
    """Field offsets and sizes: on the device, and the same on the host (kept alive by the caller)."""
    vocab = np.asarray(vocab, np.int64)
    offs = np.concatenate([[0], np.cumsum(vocab)[:-1]]).astype(np.int64)
    return _dev(offs, np.int64), _dev(vocab, np.int64), offs, vocab


def ref_pack(dims, layers, in_rows=None):
    """rs_mlp_prepare's image: per layer, for output tile t and k-group g a 1 KB block in which lane l holds
    W[16 g + 4 (l >> 4) + j][16 t + (l & 15)], j = 0..3 (zero outside K x N; layer 0's row through in_rows); then per
    layer bias [Np] and alpha [Np], zero-padded."""
    img, par = [], []
    for l, (W, b, al) in enumerate(layers):
        K, N = dims[l], dims[l + 1]
        Kp, Np = rup(K, 16), rup(N, 16)
        rows = np.asarray(in_rows) if (l == 0 and in_rows is not None) else np.arange(Kp)
        ok = (rows >= 0) & (rows < K)
        Wp = np.zeros((Kp, Np), F32)
        Wp[ok, :N] = np.asarray(W, F32)[rows[ok]]
        t, g, ln, j = np.meshgrid(np.arange(Np // 16), np.arange(Kp // 16), np.arange(64), np.arange(4), indexing="ij")
        img.append(Wp[16 * g + 4 * (ln >> 4) + j, 16 * t + (ln & 15)].reshape(-1))
        for v in (b, al):
            p = np.zeros(Np, F32)
            if v is not None:
                p[:N] = v
            par.append(p)
    return np.concatenate(img + par)


def _tower_prepare(dims, layers, in_rows=None):
    """rs_mlp_prepare into a NaN-filled buffer: every element written, bitwise the restated image."""
    L, ci = len(dims) - 1, _ci(dims)
    size = _lib.lib().rs_mlp_prepared_size(L, ci)
    assert size == mlp_geom(dims)["total"]
    prep = _nan(size)
    cols = [[None if t is None else _dev(t) for t in col] for col in zip(*layers)]
    pa = lambda ts: (C.c_void_p * L)(*[_pn(t) for t in ts]) if any(t is not None for t in ts) else None
    rows = None if in_rows is None else _dev(in_rows, np.int32)
    _lib.call("rs_mlp_prepare", L, ci, pa(cols[0]), pa(cols[1]), pa(cols[2]), _pn(rows), prep.data_ptr(), _lib.stream())
    assert np.array_equal(prep.cpu().numpy(), ref_pack(dims, layers, in_rows)), "rs_mlp_prepare: not the packed image"
    return prep, ci


# ------------------------------------------------------------------- tower
@pytest.mark.gpu
@pytest.mark.parametrize("c", TOWER_CASES, ids=lambda c: c["name"])
def test_tower_fwd(gpu, c):
    """rs_mlp_fwd / rs_mlp_affine_fwd / rs_mlp_affine_pieces_fwd under both RS_OPT_MLP_UNROLL values.  The branch of
    each case is tower_branch(dims) (asserted on the CPU, test_every_launch_line_is_named_by_a_case): widths 1 / 15 /
    16 / 17 / 1008 / 1024 as input and as hidden width; L = 1 and 8; the four activations within one tower; the four
    (8, 2) tail families exact and padded, with the trailing 1 -> 1 layer; the near-misses; narrow layers (1, 2, 3
    output tiles x 1, 2, 3 k-groups, 16 and 5 slices of a long K); the 160 KB tower; head 0 / 1, extra absent /
    present with c0, c1 != 1; bias / alpha absent; in_rows with -1 entries against the permuted kernel; the affine
    entry against BatchNormalization + tower and bitwise against rs_affine_act + rs_mlp_fwd; the pieces entry with an
    id piece, a dense piece and x absent / present (NaN in x under the pieces' columns), ids of every kind, clean and
    with one out-of-range id."""
    st, lb = _lib.stream(), _lib.lib()
    a, ref, _ = tower_inputs(c)
    dims, M, L, head = c["dims"], c["M"], len(c["dims"]) - 1, c["head"]
    K0, NL = dims[0], dims[-1]
    prep, ci = _tower_prepare(dims, a["layers"], a.get("in_rows"))
    acts = _ci(c["acts"])
    ed = None if a["extra"] is None else _dev(a["extra"])
    tail = (head, _pn(ed), a["c0"], a["c1"], M, st)
    entry = {"plain": "rs_mlp_fwd", "affine": "rs_mlp_affine_fwd", "pieces": "rs_mlp_affine_pieces_fwd"}[c["mode"]]
    check = _rel if head else _close
    if c["mode"] != "pieces":
        xd = _rows(a["x"], 3)
        aff = () if c["mode"] == "plain" else (_dev(a["scale"]), _dev(a["shift"]))
        got = {}
        for unroll in (1, 0):
            def run():
                y = _out(M, NL, 2)
                _lib.call(entry, xd.data_ptr(), K0 + 3, *[t.data_ptr() for t in aff], L, ci, acts, prep.data_ptr(),
                          y.data_ptr(), NL + 2, *tail)
                return (y,)

            with _option(_lib.OPT_MLP_UNROLL, unroll):
                got[unroll] = _twice(run)[0]
            check(entry, _get(got[unroll], NL), ref.reshape(M, NL), f"{c['name']} unroll={unroll}")
        if aff:  # the staging's affine is rs_affine_act's arithmetic: the two launches agree bit for bit
            xn, y = _out(M, K0, 1), _out(M, NL, 2)
            _lib.call("rs_affine_act", xd.data_ptr(), K0 + 3, aff[0].data_ptr(), aff[1].data_ptr(), None, 0,
                      xn.data_ptr(), K0 + 1, M, K0, st)
            _lib.call("rs_mlp_fwd", xn.data_ptr(), K0 + 1, L, ci, acts, prep.data_ptr(), y.data_ptr(), NL + 2, *tail)
            assert torch.equal(y, got[1]), "rs_mlp_affine_fwd is not rs_affine_act + rs_mlp_fwd"
        return
    sd, hd = _dev(a["scale"]), _dev(a["shift"])
    plan = a["plan"]
    n = len(plan)
    xh = a["x"].copy()
    for w, col, _ in plan:
        xh[:, col:col + w] = np.nan  # never read
    xd = _rows(xh, 3) if c["x"] else None
    arr = lambda ct, vals: (ct * n)(*vals)
    for ki, (dtype, kind) in enumerate(KINDS):
        clean = None
        for bad in (None, 0, 1):
            ab, refb, flag_want = tower_inputs(c, F64, bad)
            tabs = [None if t is None else _dev(t) for t in ab["tables"]]
            srcs = [_ids_dev(i[:, None], dtype) if i is not None else _rows(v, 1)
                    for i, v in zip(ab["ids"], ab["vals"])]
            strides = [3 if s else w + 1 for w, _, s in plan]
            for unroll in (1, 0) if bad is None else (ki % 2,):
                def run():
                    flag, y = _flag(), _out(M, NL, 2)
                    _lib.call(entry, _pn(xd), K0 + 3 if c["x"] else 0, sd.data_ptr(), hd.data_ptr(), L, ci, acts,
                              prep.data_ptr(), y.data_ptr(), NL + 2, *tail[:-1], n, arr(C.c_int, [p[0] for p in plan]),
                              arr(C.c_int, [p[1] for p in plan]), arr(C.c_int, [kind if p[2] else -1 for p in plan]),
                              arr(C.c_void_p, [s.data_ptr() for s in srcs]), arr(C.c_int64, strides),
                              arr(C.c_void_p, [_pn(t) for t in tabs]),
                              arr(C.c_int64, [PIECE_VOCAB if p[2] else 0 for p in plan]), flag.data_ptr(), st)
                    return flag, y

                with _option(_lib.OPT_MLP_UNROLL, unroll):
                    flag, y = _twice(run)
                what = f"{c['name']} kind={kind} bad={bad} unroll={unroll}"
                assert int(flag.item()) == flag_want, "error flag " + what
                got = _get(y, NL)
                check(entry, got, refb.reshape(M, NL), what)
                if bad is None and unroll == 1:
                    clean = got
                elif bad is not None and unroll == 1:
                    keep = np.arange(M) != (M - 1 if bad else 0)
                    assert np.array_equal(got[keep], clean[keep]), "a bad id changed another sample " + what


# ------------------------------------------------------------------ DeepFM
def _fused_rows(nd, F, k):
    """The fused kernels' LDS column order [emb F k | dense nd] -> Keras rows (rs_capi.h, rs_deepfm_fwd)."""
    rows = np.full(rup(nd + F * k, 16), -1, np.int32)
    rows[:F * k] = np.arange(F * k) + nd
    rows[F * k:F * k + nd] = np.arange(nd)
    return rows


@pytest.mark.gpu
@pytest.mark.parametrize("c", DEEPFM_CASES, ids=lambda c: c["name"])
def test_deepfm_fwd(gpu, c):
    """rs_deepfm_fwd_hm under every RS_OPT_DEEPFM_KERNEL value of the case (0, 1, 2 and 3 at the shapes that have
    the four forms) and rs_deepfm_fwd; the kernel of each (case, entry, option) is deepfm_branch(...) (asserted on
    the CPU, test_deepfm_and_dcn_cases_take_the_branches_their_names_say).  Output: the relative contract; FM logit:
    SUM_TOL * sum |terms|.  The two entries agree bit for bit where deepfm_branch names the same kernel for both (no
    kernel-argument metadata: more than 32 fields, or more than 16 dense k-steps)."""
    st, lb = _lib.stream(), _lib.lib()
    nd, F, k, kfm, B, dims = c["nd"], c["F"], c["k"], c["kfm"], c["B"], c["dims"]
    a, ref, fm = deepfm_inputs(c)
    L = len(dims) - 1
    td, dd, w0d = _dev(a["table"]), (_rows(a["dense"], 3) if nd else None), _dev(a["w0"])
    offd, vocd, hoff, hvoc = _meta(a["vocab"])
    fmprep = _nan(lb.rs_fm_prepared_size(nd, F, k, kfm))
    w1d, vd = _dev(a["w1"]), _dev(a["v"])  # (named: a temporary's block would be handed to the next allocation)
    _lib.call("rs_fm_prepare", w1d.data_ptr(), vd.data_ptr(), nd, F, k, kfm, fmprep.data_ptr(), st)
    prep, ci = _tower_prepare(dims, a["layers"], _fused_rows(nd, F, k))
    acts = _ci(c["acts"])
    combos = [(True, o) for o in c["opts"]] + [(False, 0)]
    name = lambda hm, opt: deepfm_branch(nd, F, k, kfm, dims, hm, opt)

    def launch(idd, kind, hm, opt, with_flag=True):
        def run():
            flag, out, lg = _flag(), _out(1, B, 2), (_out(1, B, 2) if c["logit"] else None)
            host = (hoff.ctypes.data, hvoc.ctypes.data) if hm else ()
            _lib.call("rs_deepfm_fwd_hm" if hm else "rs_deepfm_fwd", idd.data_ptr(), kind, F + 2, _pn(dd), nd + 3, nd,
                      td.data_ptr(), offd.data_ptr(), vocd.data_ptr(), *host, F, k, fmprep.data_ptr(), w0d.data_ptr(),
                      kfm, L, ci, acts, prep.data_ptr(), c["c0"], c["c1"], out.data_ptr(), _pn(lg), B,
                      flag.data_ptr() if with_flag else None, st)
            return (flag, out) + ((lg,) if c["logit"] else ())

        with _option(_lib.OPT_DEEPFM_KERNEL, opt):
            return _twice(run)

    def check(res, ref, fm, absum, what):
        entry = "rs_deepfm_fwd_hm" if what[0] else "rs_deepfm_fwd"
        _rel(entry, _get(res[1], B)[0], ref, str(what))
        if c["logit"]:
            _sum_close(entry, _get(res[2], B)[0], fm, absum, "FM logit " + str(what))

    for ki, (dtype, kind) in enumerate(KINDS):
        idd, clean = _ids_dev(a["ids"], dtype), {}
        for hm, opt in combos:
            res = clean[hm, opt] = launch(idd, kind, hm, opt)
            what = (hm, opt, name(hm, opt), c["name"], kind)
            assert int(res[0].item()) == 0, ("error flag", what)
            check(res, ref, fm, a["fm_abs"], what)
        for hm, opt in combos[:-1]:
            if name(hm, opt) == name(False, 0):
                assert all(torch.equal(x, y) for x, y in zip(clean[hm, opt], clean[False, 0])), \
                    ("the same kernel, another result", c["name"], opt)
        for bad in (0, 1):
            hm, opt = combos[(2 * ki + bad) % len(combos)]
            ab, refb, fmb = deepfm_inputs(c, F64, bad)
            idb = _ids_dev(ab["ids"], dtype)
            res = launch(idb, kind, hm, opt)
            what = (hm, opt, name(hm, opt), c["name"], kind, "bad", bad)
            assert int(res[0].item()) == _lib.FLAG_BAD_ID, ("error flag", what)
            check(res, refb, fmb, ab["fm_abs"], what)
            keep = np.arange(B) != ab["bad_row"]
            for x, y in zip(res[1:], clean[hm, opt][1:]):
                assert np.array_equal(_get(x)[0, :B][keep], _get(y)[0, :B][keep]), \
                    ("a bad id changed another sample", what)
            # err_flag = NULL (rs_capi.h: "if err_flag != NULL"; flag_error tests the pointer): the same outputs
            assert all(torch.equal(x, y) for x, y in zip(res[1:], launch(idb, kind, hm, opt, False)[1:])), \
                ("err_flag = NULL changes an output", what)


# --------------------------------------------------------------------- DCN
@pytest.mark.gpu
@pytest.mark.parametrize("c", DCN_CASES, ids=lambda c: c["name"])
def test_dcn_fwd(gpu, c):
    """rs_dcn_fwd_hm and rs_dcn_fwd under both RS_OPT_CROSS_KERNEL values; the kernel of each (case, entry, option)
    is dcn_branch(...) (asserted on the CPU).  rs_capi.h promises the two entries bit-identical; RS_OPT_CROSS_KERNEL's
    text narrows that to option 1 (the staged-tile contraction; option 0 sums G in another order), and the split-K
    tail, which only the _hm entry takes, sums a layer's k-groups in another order than the one-role tower.  So:
    bitwise where the two entries run the same tower form under option 1 or without metadata (k != 16, more than 32
    fields), the contract otherwise."""
    st, lb = _lib.stream(), _lib.lib()
    nd, F, k, Lc, B, dims = c["nd"], c["F"], c["k"], c["n_cross"], c["B"], c["dims"]
    a, ref, alpha = dcn_inputs(c)
    assert np.abs(alpha).max() < 10.0
    d, L = nd + F * k, len(dims) - 1
    td, dd = _dev(a["table"]), (_rows(a["dense"], 3) if nd else None)
    offd, vocd, hoff, hvoc = _meta(a["vocab"])
    cprep = _nan(lb.rs_cross_prepared_size(d, Lc + 1))
    Wd = _dev(np.concatenate([a["cw"], a["wo"][None]]))
    Bd = _dev(np.concatenate([a["cb"], np.zeros((1, d), F32)]))
    _lib.call("rs_cross_prepare", Wd.data_ptr(), Bd.data_ptr(), d, Lc + 1, cprep.data_ptr(), st)
    prep, ci = _tower_prepare(dims, a["layers"])
    acts = _ci(c["acts"])
    combos = [(hm, o) for hm in (True, False) for o in (0, 1)]
    name = lambda hm, opt: dcn_branch(nd, F, k, Lc, dims, hm, opt)

    def launch(idd, kind, hm, opt, with_flag=True):
        def run():
            flag, out = _flag(), _out(1, B, 2)
            host = (hoff.ctypes.data, hvoc.ctypes.data) if hm else ()
            _lib.call("rs_dcn_fwd_hm" if hm else "rs_dcn_fwd", idd.data_ptr(), kind, F + 2, _pn(dd), nd + 3, nd,
                      td.data_ptr(), offd.data_ptr(), vocd.data_ptr(), *host, F, k, Lc, cprep.data_ptr(), L, ci, acts,
                      prep.data_ptr(), out.data_ptr(), B, flag.data_ptr() if with_flag else None, st)
            return flag, out

        with _option(_lib.OPT_CROSS_KERNEL, opt):
            return _twice(run)

    for ki, (dtype, kind) in enumerate(KINDS):
        idd, clean = _ids_dev(a["ids"], dtype), {}
        for hm, opt in combos:
            flag, out = clean[hm, opt] = launch(idd, kind, hm, opt)
            what = (hm, opt, name(hm, opt), c["name"], kind)
            assert int(flag.item()) == 0, ("error flag", what)
            _rel("rs_dcn_fwd_hm" if hm else "rs_dcn_fwd", _get(out, B)[0], ref, str(what))
        assert torch.equal(clean[False, 0][1], clean[False, 1][1])  # the plain entry has one form
        for opt in (0, 1):
            same = name(True, opt) == name(False, opt) or \
                (opt == 1 and name(True, 1).replace("_ka", "") == name(False, 1))  # the staged tile, the one-role tower
            if same:
                assert torch.equal(clean[True, opt][1], clean[False, opt][1]), \
                    ("rs_dcn_fwd_hm is not bit-identical to rs_dcn_fwd", c["name"], opt, name(True, opt))
        for bad in (0, 1):
            hm, opt = combos[(2 * ki + bad) % len(combos)]
            ab, refb, _ = dcn_inputs(c, F64, bad)
            idb = _ids_dev(ab["ids"], dtype)
            flag, out = launch(idb, kind, hm, opt)
            what = (hm, opt, name(hm, opt), c["name"], kind, "bad", bad)
            assert int(flag.item()) == _lib.FLAG_BAD_ID, ("error flag", what)
            _rel("rs_dcn_fwd_hm" if hm else "rs_dcn_fwd", _get(out, B)[0], refb, str(what))
            keep = np.arange(B) != ab["bad_row"]
            assert np.array_equal(_get(out)[0, :B][keep], _get(clean[hm, opt][1])[0, :B][keep]), \
                ("a bad id changed another sample", what)
            assert torch.equal(out, launch(idb, kind, hm, opt, False)[1]), ("err_flag = NULL changes the output", what)


# --------------------------------------------------------------------- DIN
@pytest.mark.gpu
@pytest.mark.parametrize("c", DIN_CASES, ids=lambda c: c["name"])
def test_din_forward_ids(gpu, c):
    """rs_din_forward_ids; the kernel and the LDS layout of each case are din_branch(...) (asserted on the CPU): k 4 /
    8 / 16; T = 48 | 49 on the two sides of the tbase choice at k 8; T = 97, 100, 112 the NTT = 7 form and 96 / 113
    beside it; T = 1 and 128 the ends; dims[0] = 2k (no piece: n_pieces = 0) and 64; pooled absent / present; an
    out-of-range id (== vocab in the last sample, -1 in the first) in the history, the candidate and a piece; sample
    0's history is all padding (it averages its keys), sample 1's has none.  y and pooled against the float64
    reference, and bit for bit against the two launches rs_din_attention_ids_cand_fwd + rs_mlp_affine_pieces_fwd
    (rs_mlp_affine_fwd where there is no piece), as rs_capi.h promises.  err_flag is required here (a null one is
    refused)."""
    st, lb = _lib.stream(), _lib.lib()
    T, k, B, dims = c["T"], c["k"], c["B"], c["dims"]
    H1, H2 = DIN_H
    a, ref, pooled_ref = din_inputs(c)
    L, K0, NL = len(dims) - 1, dims[0], 1
    aprep = _nan(lb.rs_din_prepared_size(T, k, H1, H2))
    att = [_dev(t) for t in a["att"]]
    _lib.call("rs_din_prepare", att[0].data_ptr(), att[1].data_ptr(), att[2].data_ptr(), H1, att[3].data_ptr(),
              att[4].data_ptr(), att[5].data_ptr(), H2, att[6].data_ptr(), att[7].data_ptr(), T, k, aprep.data_ptr(),
              st)
    prep, ci = _tower_prepare(dims, a["layers"])
    acts = _ci(c["acts"])
    td, sd, hd, ptd = _dev(a["table"]), _dev(a["scale"]), _dev(a["shift"]), _dev(a["ptable"])
    plan = a["plan"]
    n = len(plan)
    arr = lambda ct, vals: (ct * n)(*vals) if n else None
    check = _rel if c["acts"][-1] == 3 else _close
    _refused(lb.rs_din_forward_ids(_p(1), 0, T, _p(2), 1, T, k, _p(3), DIN_VOCAB, H1, H2, _p(4), None, 0, _p(5), _p(6),
                                   L, ci, acts, _p(7), _p(8), 1, 0, None, None, None, None, None, None, None, B, None,
                                   None),
             b"rs_din_forward_ids", b"null pointer")
    pos = lambda v: v > 0  # a float id of 0.25 would still be the padding id 0; keep the padding exact
    for ki, (dtype, kind) in enumerate(KINDS):
        clean = None
        for bad in (None, "hist", "hist-", "cand", "cand-") + (("piece", "piece-") if n else ()):
            ab, refb, pooledb = din_inputs(c, F64, bad)
            hist, cand = _ids_dev(ab["hist"], dtype, pos), _ids_dev(ab["cand"][:, None], dtype)
            srcs = [_ids_dev(ab["pids"][:, None], dtype), _rows(ab["pvals"], 1)][:n]
            pieces = (n, arr(C.c_int, [p[0] for p in plan]), arr(C.c_int, [p[1] for p in plan]),
                      arr(C.c_int, [kind if p[2] else -1 for p in plan]), arr(C.c_void_p, [s.data_ptr() for s in srcs]),
                      arr(C.c_int64, [3 if p[2] else p[0] + 1 for p in plan]),
                      arr(C.c_void_p, [ptd.data_ptr() if p[2] else None for p in plan]),
                      arr(C.c_int64, [PIECE_VOCAB if p[2] else 0 for p in plan]))
            front = (hist.data_ptr(), kind, T + 2, cand.data_ptr(), 3, T, k, td.data_ptr(), DIN_VOCAB, H1, H2,
                     aprep.data_ptr())

            def run():
                flag, y, pooled = _flag(), _out(B, 1, 2), (_out(B, k, 3) if c["pooled"] else None)
                _lib.call("rs_din_forward_ids", *front, _pn(pooled), k + 3, sd.data_ptr(), hd.data_ptr(), L, ci, acts,
                          prep.data_ptr(), y.data_ptr(), 3, *pieces, B, flag.data_ptr(), st)
                return (flag, y) + ((pooled,) if c["pooled"] else ())

            res = _twice(run)
            what = f"{c['name']} kind={kind} bad={bad} {din_branch(T, k, H1, H2, dims)}"
            assert int(res[0].item()) == (_lib.FLAG_BAD_ID if bad else 0), "error flag " + what
            y = _get(res[1], 1)[:, 0]
            check("rs_din_forward_ids", y, refb, what)
            if c["pooled"]:
                _close("rs_din_forward_ids", _get(res[2], k), pooledb, "pooled " + what)
            if bad is None:
                clean = y
            else:
                keep = np.arange(B) != ab["bad_row"]
                assert np.array_equal(y[keep], clean[keep]), "a bad id changed another sample " + what
            if bad in (None, "hist", "cand-", "piece"):
                # the two launches: the attention writes [pooled | cand] into the concat, the tower reads the pieces
                flag, y2, emb = _flag(), _out(B, 1, 2), _out(B, K0, 3)
                scores = _nan(B * T)
                _lib.call("rs_din_attention_ids_cand_fwd", *front, scores.data_ptr(), emb.data_ptr(), K0 + 3,
                          emb.data_ptr() + 4 * k, K0 + 3, B, flag.data_ptr(), st)
                if n:
                    _lib.call("rs_mlp_affine_pieces_fwd", emb.data_ptr(), K0 + 3, sd.data_ptr(), hd.data_ptr(), L, ci,
                              acts, prep.data_ptr(), y2.data_ptr(), 3, 0, None, 1.0, 1.0, B, *pieces, flag.data_ptr(),
                              st)
                else:
                    _lib.call("rs_mlp_affine_fwd", emb.data_ptr(), K0 + 3, sd.data_ptr(), hd.data_ptr(), L, ci, acts,
                              prep.data_ptr(), y2.data_ptr(), 3, 0, None, 1.0, 1.0, B, st)
                assert torch.equal(y2, res[1]), "not bit-identical to the two launches " + what
                assert int(flag.item()) == (_lib.FLAG_BAD_ID if bad else 0), "two-launch error flag " + what
                if c["pooled"]:
                    assert np.array_equal(_get(emb)[:, :k], _get(res[2], k)), \
                        "pooled differs from the two launches " + what


# ------------------------------------------------------------- model level
def _model_check(y, ref, ref32, what):
    """The case is conditioned (float32 oracle within RTOL / 4: the weights are the model's own initialisation, drawn
    on the device, so this is checked here), then the contract."""
    assert_rel_close(np.asarray(ref32, F64), ref, RTOL / 4, "float32 oracle of " + what)
    assert_rel_close(y, ref, RTOL, what)


@pytest.mark.gpu
@pytest.mark.parametrize("inside", [True, False])
def test_deepfm_model_at_the_fused_bound(gpu, inside):
    """DeepFM just inside ([429, 768, 112, 1]: exactly 120 KB) and just outside ([429, 768, 128, 1]) fused_ok():
    forward is the one launch inside and the two launches outside, and equals the float64 oracle on both sides."""
    import recommender_system_amd as rs
    from tests.helpers import criteo_columns, dnn_params, tables_of
    rng = np.random.default_rng(5)
    vocabs = rng.integers(2, 50, 26)
    hidden = [768, 112] if inside else [768, 128]
    m = rs.DeepFM(criteo_columns(vocabs, embed_dim=16), 10, 1e-4, 1e-4, hidden, 1, "relu", embed_dim=16, seed=0)
    assert m.fused_ok() == inside == deepfm_supported(13, 26, 16, 10, [429] + hidden + [1])
    B = 33
    dense, ids = rng.random((B, 13)).astype(F32), _ids(rng, B, vocabs)
    y = m.forward((dense, ids))
    if inside:
        assert torch.equal(y, m.forward_fused((dense, ids)))
    else:
        assert torch.equal(y, m.forward_unfused((dense, ids)))
        with pytest.raises(_lib.RSError, match="unsupported shape"):
            m.forward_fused((dense, ids))
    hidden_p, out_p = dnn_params(m.dnn)
    n = lambda t: t.detach().cpu().numpy()
    p = {"tables": tables_of(m.embed_layer), "w0": n(m.fm.w0), "w1": n(m.fm.w1), "v": n(m.fm.v),
         "dnn_hidden": hidden_p, "dnn_out": out_p}
    _model_check(y, O.deepfm(None, p, inputs=(dense, ids))[0], O.deepfm(None, p, dt=F32, inputs=(dense, ids))[0],
                 f"DeepFM.forward inside={inside}")


@pytest.mark.gpu
@pytest.mark.parametrize("inside", [True, False])
def test_dcn_model_at_the_fused_bound(gpu, inside):
    """DCN just inside ([640, 256, 112, 1]: exactly 100 KB) and just outside ([640, 256, 128, 1]) fused_ok()."""
    import recommender_system_amd as rs
    from tests.helpers import criteo_columns, dnn_params, tables_of
    rng = np.random.default_rng(6)
    vocabs = rng.integers(2, 50, 32)
    hidden = [256, 112] if inside else [256, 128]
    m = rs.DCN(criteo_columns(vocabs, n_dense=128, embed_dim=16), hidden, 1, "relu", layer_num=2, embed_dim=16, seed=3)
    assert m.fused_ok() == inside == dcn_supported(128, 32, 16, 2, [640] + hidden + [1])
    B = 17
    dense, ids = rng.random((B, 128)).astype(F32), _ids(rng, B, vocabs)
    y = m.forward((dense, ids))
    if inside:
        assert torch.equal(y, m.forward_fused((dense, ids)))
    else:
        assert torch.equal(y, m.forward_unfused((dense, ids)))
        with pytest.raises(_lib.RSError, match="unsupported shape"):
            m.forward_fused((dense, ids))
    hidden_p, out_p = dnn_params(m.dense_layer)
    n = lambda t: t.detach().cpu().numpy()
    p = {"tables": tables_of(m.embed_layer), "cross_w": [n(w) for w in m.cross_layer.cross_weight],
         "cross_b": [n(b) for b in m.cross_layer.cross_bias], "dnn_hidden": hidden_p, "dnn_out": out_p,
         "out_kernel": n(m.output_layer.kernel), "out_bias": n(m.output_layer.bias)}
    _model_check(y, O.dcn(None, p, inputs=(dense, ids))[0], O.dcn(None, p, dt=F32, inputs=(dense, ids))[0],
                 f"DCN.forward inside={inside}")
