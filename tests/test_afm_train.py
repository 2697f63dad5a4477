"""AFM training: rs_afm_train_fwd (ids -> rows -> pooled pairs -> head ->
loss gradient -> row gradients, one launch), AFM.train_step and compile_fit on
AFM, against a plain numpy float64 restatement of layer/interaction.py:322-351
+ model/afm.py:15-18 under utils/compile_fit.py:9-15.

CPU: the reference's gradients against central finite differences (a random
linear functional of the per-sample losses, step 1e-6, agreement 1e-6: the
rule of test_train_blocks part A), the arg-max precondition of every 'max' GPU
case, the entry's argument checks with dummy pointers, the CPU-model refusal.

GPU: the kernel at every lane layout (float4 lanes k % 4 == 0, scalar lanes
otherwise, an unaligned table), both 32-field chunk boundaries (F = 32, 33,
40, 70), one- and multi-workgroup grids; buffer coverage and determinism;
out-of-range ids; the forward; one train_step per mode and input form;
check_ids; compile_fit.

Tolerance: helpers.RTOL through assert_scaled_close (assert_rel_close for the
model output), as everywhere in the project.

'max' precondition: the kernel sends a tie's gradient to the first tied pair
while TF splits it, and an fp32 product within rounding of the runner-up
could pick another pair than the fp64 reference.  The fp64 product of two
fp32 rows is exact and the fp32 product is off by at most 2^-24 ~ 6e-8
relative, so a gap above 1e-6 max(|p1|, |p2|) (16x wider) cannot flip in
fp32: every 'max' case is checked for it on the reference alone, and a case
that stops meeting it fails as a precondition, not as a tolerance.
"""
import ctypes as C
import os

import numpy as np
import pytest

from recommender_system_amd import _lib
from tests.helpers import RTOL, assert_rel_close, assert_scaled_close, criteo_columns

torch = pytest.importorskip("torch")

F64, F32 = np.float64, np.float32
MODES = ("att", "avg", "max")
MODE_ID = {"att": 0, "avg": 1, "max": 2}
GAP = 1e-6
SAMPLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "criteo_train_1w.txt.gz")


# --------------------------------------------------------------------------
# The float64 reference
# --------------------------------------------------------------------------
def _sig(x):
    return 1.0 / (1.0 + np.exp(-x))


def ref_pairs(rows):
    """[B, P, k] products of the (i<j) row-major field pairs of rows [B, F, k]."""
    iu, ju = np.triu_indices(rows.shape[1], 1)
    return rows[:, iu, :] * rows[:, ju, :], iu, ju


def ref_afm(rows, w, b, t, mode, n_sig, cw=None):
    """Forward and backward of sum_b cw_b loss_b (cw = 1/B: the batch mean)
    from the looked-up rows [B, F, k]: dict of pooled, prob, loss, g, de
    [B, F, k], dw [k], db."""
    rows, w, t = np.asarray(rows, F64), np.asarray(w, F64).reshape(-1), np.asarray(t, F64)
    B, nf, k = rows.shape
    P = nf * (nf - 1) // 2
    cw = np.full(B, 1.0 / B) if cw is None else np.asarray(cw, F64)
    arg = None
    if nf < 2:
        x = np.zeros((B, k))
    else:
        prod, iu, ju = ref_pairs(rows)
        if mode == "max":
            arg = prod.argmax(1)  # the first maximum
            x = np.take_along_axis(prod, arg[:, None, :], 1)[:, 0, :]
        else:
            x = prod.sum(1) / (P if mode == "avg" else 1)
    z = x @ w + float(b)
    s = _sig(z)
    u, dz = (s, s * (1 - s)) if n_sig == 2 else (z, 1.0)
    loss = np.maximum(u, 0) - u * t + np.log1p(np.exp(-np.abs(u)))
    g = cw * (_sig(u) - t) * dz
    dx = g[:, None] * w[None, :]
    de = np.zeros_like(rows)
    if nf >= 2:
        if mode == "max":
            bi, ci = np.meshgrid(np.arange(B), np.arange(k), indexing="ij")
            i_s, j_s = iu[arg], ju[arg]
            de[bi, i_s, ci] = dx * rows[bi, j_s, ci]
            de[bi, j_s, ci] = dx * rows[bi, i_s, ci]
        else:
            de = dx[:, None, :] * (rows.sum(1, keepdims=True) - rows) / (P if mode == "avg" else 1)
    return {"pooled": x, "prob": _sig(u), "loss": loss, "g": g, "de": de, "dw": x.T @ g, "db": g.sum()}


def max_gap(rows):
    """The smallest relative gap between the largest and the second largest
    pair product over every (b, c) (inf with fewer than two pairs)."""
    rows = np.asarray(rows, F64)
    if rows.shape[1] < 3:
        return np.inf
    top = np.sort(ref_pairs(rows)[0], 1)[:, -2:, :]
    p2, p1 = top[:, 0, :], top[:, 1, :]
    return float(np.min((p1 - p2) / np.maximum(np.abs(p1), np.abs(p2))))


def assert_max_precondition(rows, what):
    gap = max_gap(rows)
    assert gap > GAP, f"{what}: 'max' precondition not met by the reference (smallest gap {gap:.3e} <= {GAP})"


def lookup(table, offs, vocabs, ids):
    """rows [B, F, k] (float64) of the concatenated table; an id outside
    [0, vocab) is the zero row."""
    ids = np.asarray(ids).astype(np.int64)
    ok = (ids >= 0) & (ids < np.asarray(vocabs)[None, :])
    rows = np.asarray(table, F64)[np.where(ok, ids, 0) + np.asarray(offs)[None, :]]
    return rows * ok[:, :, None]


def ref_step(p, ids, t, mode, lr):
    """One SGD step on p = {table, w, b} (float64, changed in place) from the
    pre-step weights; duplicates of a row add.  Returns the losses."""
    rows = lookup(p["table"], p["offs"], p["vocabs"], ids)
    r = ref_afm(rows, p["w"], p["b"], t, mode, 2)
    np.subtract.at(p["table"], (np.asarray(ids, np.int64) + p["offs"][None, :]).reshape(-1),
                   lr * r["de"].reshape(-1, rows.shape[2]))
    p["w"] = p["w"] - lr * r["dw"]
    p["b"] = p["b"] - lr * r["db"]
    return r["loss"], rows


# --------------------------------------------------------------------------
# Cases (numpy only, so the CPU tests see exactly what the GPU tests run)
# --------------------------------------------------------------------------
SHAPES_ALL = [(1, 1, 1), (3, 2, 1), (5, 3, 3), (300, 5, 4), (37, 26, 8), (37, 26, 16), (64, 26, 20), (7, 4, 33),
              (19, 32, 64)]
SHAPES_SUM = [(9, 33, 16), (6, 40, 5), (5, 70, 4)]  # 'att' / 'avg' only: beyond the 32 fields 'max' holds
KERNEL_CASES = [(s, m) for s in SHAPES_ALL for m in MODES] + [(s, m) for s in SHAPES_SUM for m in ("att", "avg")]
VARIANTS = ["i32", "i64", "f32", "strided", "unaligned", "one_sigmoid"]


def make_case(B, nf, k, seed=0):
    """Rows uniform in +-0.5, head kernel N(0,1), bias in +-0.5, vocabularies
    of 3..7 per field (duplicate rows occur).  Seed 0 meets the 'max'
    precondition at every shape used here (test_max_precondition_of_every_gpu_case)."""
    rng = np.random.default_rng(seed)
    vocabs = rng.integers(3, 8, nf)
    offs = np.concatenate([[0], np.cumsum(vocabs)[:-1]]).astype(np.int64)
    return {"vocabs": vocabs.astype(np.int64), "offs": offs,
            "table": rng.uniform(-0.5, 0.5, (int(vocabs.sum()), k)).astype(F32),
            "w": rng.normal(size=k).astype(F32), "b": rng.uniform(-0.5, 0.5, 1).astype(F32),
            "ids": np.stack([rng.integers(0, v, B) for v in vocabs], 1).astype(np.int64),
            "t": rng.integers(0, 2, B).astype(F32), "k": k}


def case_rows(c, ids=None):
    return lookup(c["table"], c["offs"], c["vocabs"], c["ids"] if ids is None else ids)


def bad_id_case():
    c = make_case(37, 26, 16)
    bad = c["ids"].copy()
    bad[11, 4] = c["vocabs"][4]
    return c, bad


STEP_SHAPE = (24, 26, 16)


def criteo_case(mode):
    """The first 96 rows of the bundled Criteo sample, a table in +-0.05 (the
    Keras init's range) and the head, all from numpy."""
    from recommender_system_amd.dataset import criteo_compact, features_dict
    dense, ids, label, _ = criteo_compact(SAMPLE)
    cols = features_dict(SAMPLE, embed_dim=8)
    vocabs = np.array([f["feat_onehot_dim"] for f in cols[1]], np.int64)
    rng = np.random.default_rng(3)
    offs = np.concatenate([[0], np.cumsum(vocabs)[:-1]]).astype(np.int64)
    return {"cols": cols, "dense": dense[:96].astype(F32), "ids": ids[:96], "t": label[:96].astype(F32),
            "vocabs": vocabs, "offs": offs, "table": rng.uniform(-0.05, 0.05, (int(vocabs.sum()), 8)).astype(F32),
            "w": rng.normal(size=8).astype(F32), "b": rng.uniform(-0.5, 0.5, 1).astype(F32), "k": 8}


def criteo_ref_loop(c, mode, lr=0.1, batch=32, epochs=2):
    """compile_fit's loop in float64: the per-epoch mean losses; checks the
    'max' precondition on the rows of every step."""
    p = {"table": c["table"].astype(F64), "w": c["w"].astype(F64), "b": float(c["b"][0]), "offs": c["offs"],
         "vocabs": c["vocabs"]}
    hist = []
    for ep in range(epochs):
        losses = []
        for r0 in range(0, 96, batch):
            loss, rows = ref_step(p, c["ids"][r0:r0 + batch], c["t"][r0:r0 + batch], mode, lr)
            if mode == "max":
                assert_max_precondition(rows, f"compile_fit epoch {ep} rows {r0}..")
            losses.append(loss)
        hist.append(float(np.concatenate(losses).mean()))
    return hist


# --------------------------------------------------------------------------
# CPU
# --------------------------------------------------------------------------
def _fd(f, x, h=1e-6):
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
    g = np.asarray(g, F64)
    rms = float(np.sqrt(np.mean(g ** 2)))
    bad = ~(np.abs(fd - g) <= 1e-6 * np.maximum(np.abs(g), rms) + 1e-300)
    assert not bad.any(), f"{what}: finite differences off by {float(np.max(np.abs(fd - g))):.3e}"


@pytest.mark.parametrize("n_sig", [1, 2])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("nf", [1, 2, 5])
def test_reference_gradients_match_finite_differences(mode, n_sig, nf):
    rng = np.random.default_rng(10 * nf + n_sig)
    B, k = 4, 3
    rows = rng.uniform(-0.5, 0.5, (B, nf, k))
    w, b, t = rng.normal(size=k), rng.uniform(-0.5, 0.5, 1), rng.integers(0, 2, B).astype(F64)
    cw = rng.normal(size=B)
    if mode == "max":  # the arg-max must not move under the +-1e-6 probes
        assert max_gap(rows) > 1e-3
    f = lambda: float((cw * ref_afm(rows, w, b[0], t, mode, n_sig, cw)["loss"]).sum())
    r = ref_afm(rows, w, b[0], t, mode, n_sig, cw)
    _fd_close(_fd(f, rows), r["de"], f"{mode} de")
    _fd_close(_fd(f, w), r["dw"], f"{mode} dw")
    _fd_close(_fd(f, b), np.array([r["db"]]), f"{mode} db")
    if nf == 1:
        assert not r["pooled"].any() and not r["de"].any() and not r["dw"].any() and r["db"] != 0


def test_max_precondition_of_every_gpu_case():
    for B, nf, k in SHAPES_ALL + [STEP_SHAPE]:
        assert_max_precondition(case_rows(make_case(B, nf, k)), f"case {(B, nf, k)}")
    c, bad = bad_id_case()
    assert_max_precondition(case_rows(c, bad), "bad-id case")
    criteo_ref_loop(criteo_case("max"), "max")


def _entry(**kw):
    """rs_afm_train_fwd with dummy non-null pointers (no device): returns the status."""
    one = C.c_void_p(16)
    a = dict(ids=one, id_kind=0, id_stride=26, table=one, offs=one, vocab=one, F=26, k=16, mode=0, w=one, b=one,
             n_sig=2, labels=one, batch=0, pooled=one, ps=16, prob=None, g=one, loss=None, drows=one, ds=26 * 16)
    a.update(kw)
    return _lib.lib().rs_afm_train_fwd(a["ids"], a["id_kind"], a["id_stride"], a["table"], a["offs"], a["vocab"],
                                       a["F"], a["k"], a["mode"], a["w"], a["b"], a["n_sig"], a["labels"], a["batch"],
                                       a["pooled"], a["ps"], a["prob"], a["g"], a["loss"], a["drows"], a["ds"], None,
                                       None)


def test_argument_checks_without_device():
    assert _entry(batch=0) == 0  # RS_OK, nothing launched
    assert _entry(batch=0, k=65) == 0
    for what, kw in [("k = 65", dict(k=65, ps=65, ds=26 * 65)), ("mode = 3", dict(mode=3)),
                     ("'max' with 33 fields", dict(mode=2, F=33, ds=33 * 16)), ("n_sigmoid = 0", dict(n_sig=0)),
                     ("n_sigmoid = 3", dict(n_sig=3)), ("null ids", dict(ids=None)), ("null table", dict(table=None)),
                     ("null g", dict(g=None)), ("null drows", dict(drows=None))]:
        assert _entry(batch=4, **kw) == -1, f"{what} accepted"
        assert b"rs_afm_train_fwd" in _lib.lib().rs_last_error_string(), what
    assert _entry(batch=4, mode=2, F=33, ds=33 * 16) == -1
    assert b"at most 32 fields" in _lib.lib().rs_last_error_string()


def test_train_step_needs_a_hip_device():
    import recommender_system_amd as rs
    m = rs.AFM(criteo_columns([5, 3], n_dense=2, embed_dim=4), "max", device="cpu", seed=0)
    with pytest.raises(NotImplementedError, match="AFM.train_step: training runs only on a HIP device"):
        m.train_step(np.zeros((2, 4)), np.zeros(2))


# --------------------------------------------------------------------------
# GPU
# --------------------------------------------------------------------------
gpu_test = pytest.mark.gpu


def _dev(a, gpu):
    return torch.as_tensor(np.ascontiguousarray(a), device=gpu)


def run_entry(gpu, c, mode, ids=None, n_sig=2, id_dtype=np.int64, id_stride=None, unaligned=False, fill=None):
    """One rs_afm_train_fwd launch on case c: dict of numpy outputs and the flag."""
    ids = c["ids"] if ids is None else ids
    B, nf = ids.shape
    k = c["k"]
    if id_stride is None:
        idt = _dev(ids.astype(id_dtype), gpu)
    else:  # a [B, id_stride] matrix whose last F columns are the ids (the packed X)
        X = np.full((B, id_stride), 1e9, id_dtype)
        X[:, id_stride - nf:] = ids
        idt = _dev(X, gpu)[:, id_stride - nf:]
    table = c["table"]
    if unaligned:  # the table one float past a 16-byte boundary
        buf = torch.zeros(table.size + 1, dtype=torch.float32, device=gpu)
        buf[1:] = _dev(table.reshape(-1), gpu)
        tt = buf[1:]
        assert tt.data_ptr() % 16 == 4
    else:
        tt = _dev(table, gpu)
    offs, vocab = _dev(c["offs"], gpu), _dev(c["vocabs"], gpu)
    w, b, t = _dev(c["w"], gpu), _dev(c["b"], gpu), _dev(c["t"], gpu)
    new = lambda *shape: torch.full(shape, float("nan") if fill is None else fill, dtype=torch.float32, device=gpu)
    pooled, prob, g, loss, de = new(B, k), new(B), new(B), new(B), new(B, nf * k)
    flag = torch.zeros(1, dtype=torch.int32, device=gpu)
    _lib.call("rs_afm_train_fwd", idt.data_ptr(), _lib.id_kind(idt), idt.stride(0), tt.data_ptr(), offs.data_ptr(),
              vocab.data_ptr(), nf, k, MODE_ID[mode], w.data_ptr(), b.data_ptr(), n_sig, t.data_ptr(), B,
              pooled.data_ptr(), k, prob.data_ptr(), g.data_ptr(), loss.data_ptr(), de.data_ptr(), nf * k,
              flag.data_ptr(), _lib.stream())
    torch.cuda.synchronize()
    out = {n: v.cpu().numpy() for n, v in (("pooled", pooled), ("prob", prob), ("g", g), ("loss", loss), ("de", de))}
    out["flag"] = int(flag.item())
    return out


def check_against_reference(out, rows, c, mode, n_sig, what):
    r = ref_afm(rows, c["w"], c["b"][0], c["t"], mode, n_sig)
    B = rows.shape[0]
    assert_scaled_close(out["pooled"], r["pooled"], RTOL, f"{what} pooled")
    assert_rel_close(out["prob"], r["prob"], RTOL, f"{what} prob")
    assert_scaled_close(out["g"], r["g"], RTOL, f"{what} g")
    assert_scaled_close(out["loss"], r["loss"], RTOL, f"{what} loss")
    assert_scaled_close(out["de"], r["de"].reshape(B, -1), RTOL, f"{what} drows")


@gpu_test
@pytest.mark.parametrize("shape,mode", KERNEL_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else v)
def test_kernel_matches_reference(gpu, shape, mode):
    c = make_case(*shape)
    rows = case_rows(c)
    if mode == "max":
        assert_max_precondition(rows, f"case {shape}")
    out = run_entry(gpu, c, mode)
    assert out["flag"] == 0
    check_against_reference(out, rows, c, mode, 2, f"{shape} {mode}")


@gpu_test
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("variant", VARIANTS)
def test_kernel_variants(gpu, variant, mode):
    c = make_case(37, 26, 16)
    rows = case_rows(c)
    if mode == "max":
        assert_max_precondition(rows, "case (37, 26, 16)")
    kw = {"i32": dict(id_dtype=np.int32), "i64": dict(id_dtype=np.int64), "f32": dict(id_dtype=F32),
          "strided": dict(id_dtype=F32, id_stride=39), "unaligned": dict(unaligned=True),
          "one_sigmoid": dict(n_sig=1)}[variant]
    out = run_entry(gpu, c, mode, **kw)
    assert out["flag"] == 0
    check_against_reference(out, rows, c, mode, kw.get("n_sig", 2), f"{variant} {mode}")


@gpu_test
@pytest.mark.parametrize("shape,mode", [((37, 26, 16), "att"), ((37, 26, 16), "max"), ((64, 26, 20), "avg"),
                                        ((64, 26, 20), "max"), ((9, 33, 16), "att"), ((5, 70, 4), "avg")],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else v)
def test_every_element_written_and_bit_identical(gpu, shape, mode):
    """drows, pooled and g come back finite everywhere from NaN-filled
    buffers, and from differently filled buffers bit for bit the same."""
    c = make_case(*shape)
    a = run_entry(gpu, c, mode)
    b = run_entry(gpu, c, mode, fill=7.0)
    for n in ("de", "pooled", "g", "prob", "loss"):
        assert np.isfinite(a[n]).all(), f"{n}: an element was not written"
        assert np.array_equal(a[n], b[n]), f"{n}: two runs differ"


@gpu_test
@pytest.mark.parametrize("mode", MODES)
def test_out_of_range_id(gpu, mode):
    c, bad = bad_id_case()
    rows = case_rows(c, bad)  # the bad id's row taken as zero
    assert not rows[11, 4].any()
    if mode == "max":
        assert_max_precondition(rows, "bad-id case")
    out = run_entry(gpu, c, mode, ids=bad)
    assert out["flag"] & _lib.FLAG_BAD_ID
    k = c["k"]
    assert not out["de"][11, 4 * k:5 * k].any(), "the bad id's own block is not 0"
    r = ref_afm(rows, c["w"], c["b"][0], c["t"], mode, 2)
    ref_de = r["de"].copy()
    ref_de[11, 4] = 0  # the reference's gradient to the (nonexistent) row
    assert_scaled_close(out["de"], ref_de.reshape(37, -1), RTOL, f"{mode} drows")
    assert_scaled_close(out["pooled"], r["pooled"], RTOL, f"{mode} pooled")
    assert_scaled_close(out["g"], r["g"], RTOL, f"{mode} g")


def _model(gpu, c, mode, nd=0):
    """AFM with case c's weights (and the reference's float64 copy of them)."""
    import recommender_system_amd as rs
    cols = c.get("cols") or criteo_columns(c["vocabs"], n_dense=nd, embed_dim=c["k"])
    m = rs.AFM(cols, mode, device=gpu, seed=5)
    L = m.afm_layer
    with torch.no_grad():
        L.embed_layer.table.copy_(_dev(c["table"], gpu))
        L.output_layer.kernel.copy_(_dev(c["w"].reshape(-1, 1), gpu))
        L.output_layer.bias.copy_(_dev(c["b"], gpu))
    m._weights_changed()
    p = {"table": c["table"].astype(F64), "w": c["w"].astype(F64), "b": float(c["b"][0]), "offs": c["offs"],
         "vocabs": c["vocabs"]}
    return m, p


@gpu_test
@pytest.mark.parametrize("mode", MODES)
def test_prob_agrees_with_forward(gpu, mode):
    c = make_case(37, 26, 16)
    m, _ = _model(gpu, c, mode)
    y = m((np.zeros((37, 0), F32), c["ids"])).reshape(-1)
    assert_rel_close(run_entry(gpu, c, mode)["prob"], y, RTOL, f"{mode} prob against AFM.forward")


def _assert_params(m, p, what):
    L = m.afm_layer
    assert_scaled_close(L.embed_layer.table, p["table"], RTOL, f"{what} table")
    assert_scaled_close(L.output_layer.kernel.reshape(-1), p["w"], RTOL, f"{what} head kernel")
    assert_scaled_close(L.output_layer.bias, np.array([p["b"]]), RTOL, f"{what} head bias")


@gpu_test
@pytest.mark.parametrize("id_dtype", [np.int32, np.int64], ids=["i32", "i64"])
@pytest.mark.parametrize("form", ["pair", "packed"])
@pytest.mark.parametrize("mode", MODES)
def test_train_step_matches_reference(gpu, mode, form, id_dtype):
    nd = 3
    c = make_case(*STEP_SHAPE)
    m, p = _model(gpu, c, mode, nd)
    if mode == "max":
        assert_max_precondition(case_rows(c), "train_step case")
    dense = np.random.default_rng(1).random((STEP_SHAPE[0], nd)).astype(F32)
    ids = c["ids"].astype(id_dtype)
    att = None
    if mode == "att":
        a = m.afm_layer.attention_layer
        att = {n: v.detach().clone() for n, v in a.keras_weights().items()}
        assert att
    inputs = (dense, ids) if form == "pair" else np.concatenate([dense, ids.astype(F32)], 1)
    loss = m.train_step(inputs, c["t"], lr=0.1, return_loss=True)
    ref_loss, _ = ref_step(p, c["ids"], c["t"], mode, 0.1)
    assert_scaled_close(loss, ref_loss, RTOL, f"{mode} losses")
    _assert_params(m, p, f"{mode} {form}")
    assert not np.array_equal(m.afm_layer.embed_layer.table.cpu().numpy(), c["table"]), "the step changed nothing"
    if att is not None:
        for n, v in m.afm_layer.attention_layer.keras_weights().items():
            assert torch.equal(v, att[n]), f"attention weight {n} changed"
    assert m.train_step(inputs, c["t"], lr=0.1) is None


@gpu_test
@pytest.mark.parametrize("mode", MODES)
def test_bad_id_changes_nothing(gpu, mode):
    c, bad = bad_id_case()
    m, p = _model(gpu, c, mode)
    before = {n: v.detach().clone() for n, v in m.keras_weights().items()}
    dense = np.zeros((37, 0), F32)
    with pytest.raises(_lib.RSError) as info:
        m.train_step((dense, bad), c["t"], lr=0.1, check_ids=True)
    assert isinstance(info.value, IndexError)  # the id check's error, as TF's Embedding raises
    for n, v in m.keras_weights().items():
        assert torch.equal(v, before[n]), f"{n} changed by a refused step"
    m.train_step((dense, c["ids"]), c["t"], lr=0.1)  # the model still trains
    ref_step(p, c["ids"], c["t"], mode, 0.1)
    _assert_params(m, p, "step after a refused one")


@gpu_test
@pytest.mark.parametrize("mode", ["att", "max"])
def test_train_step_graph_capture(gpu, mode):
    """train_step(check_ids=False) captured once and replayed twice leaves the
    weights of two eager steps on a twin, bit for bit: the entry neither
    allocates nor synchronises, and the step is a linear chain on one stream."""
    c = make_case(*STEP_SHAPE)
    (a, _), (b, _) = _model(gpu, c, mode), _model(gpu, c, mode)
    dense, ids, t = _dev(np.zeros((STEP_SHAPE[0], 0), F32), gpu), _dev(c["ids"], gpu), _dev(c["t"], gpu)
    for m in (a, b):  # one eager step each: workspaces allocated outside the capture
        m.train_step((dense, ids), t, lr=0.05, check_ids=False)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            a.train_step((dense, ids), t, lr=0.05, check_ids=False)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    for _ in range(2):
        b.train_step((dense, ids), t, lr=0.05, check_ids=False)
    torch.cuda.synchronize()
    wa, wb = a.keras_weights(), b.keras_weights()
    for n in wa:
        assert torch.equal(wa[n], wb[n]), f"{n}: replayed steps differ from eager steps"


@gpu_test
@pytest.mark.parametrize("mode", MODES)
def test_compile_fit(gpu, mode):
    """compile_fit on 96 rows of the bundled sample, batch 32, 2 epochs: the
    history is the means of train_step called by hand on a twin, bit for bit,
    and the float64 loop's within one tolerance per step taken."""
    from recommender_system_amd.train import compile_fit
    c = criteo_case(mode)
    ref_hist = criteo_ref_loop(c, mode)
    a, _ = _model(gpu, c, mode)
    b, _ = _model(gpu, c, mode)
    hist = compile_fit(a, c["dense"], c["ids"], c["t"], batch_size=32, epochs=2, sgd=0.1)
    by_hand = []
    dense, ids, t = _dev(c["dense"], gpu), _dev(c["ids"], gpu), _dev(c["t"], gpu)
    for _ in range(2):
        losses = [b.train_step((dense[r0:r0 + 32], ids[r0:r0 + 32]), t[r0:r0 + 32], lr=0.1, return_loss=True,
                               check_ids=False) for r0 in range(0, 96, 32)]
        by_hand.append(float(torch.cat(losses).mean().item()))
    assert hist == by_hand
    wa, wb = a.keras_weights(), b.keras_weights()
    for n in wa:
        assert torch.equal(wa[n], wb[n]), f"{n}: compile_fit and the steps by hand differ"
    n_steps = 6
    assert np.all(np.abs(np.array(hist) - ref_hist) <= n_steps * RTOL * np.abs(ref_hist)), (hist, ref_hist)
