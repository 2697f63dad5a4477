"""The kernarg FM kernels' instruction-fetch levers (the merged id
load of embed_fm_body's ID1 — a two-pass wave loads field w in its lower half
and field w + 16 in its upper half with one instruction and swaps the halves;
the epilogue scout was measured and not kept, its cases stay) against kernels
built without them — rs_embed_fm_fwd (the device-metadata kernel), the
struct-argument form (RS_OPT_EMBED_FM_KERNEL 4), the streamed launch — and
the fp64 oracle.  The arithmetic and its order are the same everywhere, so
kernel against kernel is bit for bit.

What such a lever could break, and the case that shows it: the two halves of
the merged id load changing places (batch 1: field w = 0, field w + 16 =
vocab - 1 in every sample; batch 0: the two ids differ in every sample), a
logit or error flag written where none is due (canary floats behind the
logits, the error word after a clean run), LDS garbage reaching an output (a
launch after a kernel that left NaNs in LDS), a bad id in a one-pass wave's
field or in a two-pass wave's second field going unreported or changing
another sample.

Shapes at k 16, FM width 10 (F, nd): (26, 13) the specialised kernel; (32, 0) no wave without a
second pass; (17, 3) exactly one two-pass wave; (16, 13) no second pass;
(9, 2) waves with no field.  B: a partial tile, a full one, two tiles with
one sample in the second, three tiles.  Ids and dense rows are column slices
of wider tensors (id stride F + 3).  The other row lengths and FM widths —
with and without the merged load — are in test_other_geometries_bit_identical."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle import ctr_oracle as O
from tests.helpers import assert_scaled_close, random_ids

K, KFM, VOCAB = 16, 10, 50
S, B_MAX, CANARY = 2, 33, 16
SHAPES = [(26, 13), (32, 0), (17, 3), (16, 13), (9, 2)]  # (F, nd)
BATCHES = [1, 16, 17, 33]


@functools.lru_cache(maxsize=None)
def _case(F, nd, idt, k=K, kfm=KFM):
    """One weight set, S x B_MAX samples and their fp64 logits per shape, id
    type and row / FM width (computed once).  Batch 0: random ids, a two-pass wave's two fields
    never equal in a sample.  Batch 1: every two-pass wave's first field 0 and
    its second field VOCAB - 1."""
    from recommender_system_amd import _lib
    dev = torch.device("cuda")
    rng = np.random.default_rng(9000 + 100 * F + nd + 7 * k + kfm)
    vocabs = [VOCAB] * F
    offs = np.arange(F, dtype=np.int64) * VOCAB
    d = nd + F * k
    table = rng.uniform(-0.05, 0.05, size=(F * VOCAB, k)).astype(np.float32)
    w1 = (rng.standard_normal((d, 1)) * 0.05).astype(np.float32)
    v = (rng.standard_normal((d, kfm)) * 0.05).astype(np.float32)
    w0 = np.array([0.031], np.float32)
    ids = np.stack([random_ids(rng, B_MAX, vocabs) for _ in range(S)])
    for w in range(max(F - 16, 0)):
        same = ids[0, :, w] == ids[0, :, w + 16]
        ids[0, same, w + 16] = (ids[0, same, w + 16] + 1) % VOCAB
        assert (ids[0, :, w] != ids[0, :, w + 16]).all()
        ids[1, :, w], ids[1, :, w + 16] = 0, VOCAB - 1
    dense = rng.random((S, B_MAX, nd)).astype(np.float32)
    tables = [table[o:o + VOCAB] for o in offs]
    ref = np.stack([O.fm_layer(np.concatenate([dense[s], O.embed_layer(ids[s], tables, np.float64)], 1),
                               w0, w1, v)[:, 0] for s in range(S)])
    t = lambda a, dt=torch.float32: torch.as_tensor(a).to(dt).to(dev).contiguous()
    c = {"F": F, "nd": nd, "k": k, "kfm": kfm, "ref": ref, "kind": 0 if idt == torch.int32 else 1,
         "table": t(table), "w0": t(w0),
         "offs": t(offs, torch.int64), "voc": t(vocabs, torch.int64), "hoff": (C.c_int64 * F)(*offs),
         "hvoc": (C.c_int64 * F)(*vocabs)}
    w1_d, v_d = t(w1), t(v)
    c["prep"] = torch.empty(_lib.lib().rs_fm_prepared_size(nd, F, k, kfm), device=dev)
    _lib.call("rs_fm_prepare", w1_d.data_ptr(), v_d.data_ptr(), nd, F, k, kfm, c["prep"].data_ptr(), 0)
    # rows wider than the data: ids in columns 1 .. 1+F of F+3, dense in 1 .. 1+nd of nd+3
    c["ids_wide"] = _wide(t(ids, idt), 1, 2, -7)
    c["dense_wide"] = _wide(t(dense), 1, 2, 99.0) if nd else None
    torch.cuda.synchronize()
    return c


def _wide(x, before, after, fill):
    w = torch.full(x.shape[:-1] + (before + x.shape[-1] + after,), fill, dtype=x.dtype, device=x.device)
    w[..., before:before + x.shape[-1]] = x
    return w


def _views(c, ids_wide=None):
    F, nd = c["F"], c["nd"]
    ids = (c["ids_wide"] if ids_wide is None else ids_wide)[:, :, 1:1 + F]
    dense = c["dense_wide"][:, :, 1:1 + nd] if nd else None
    assert ids.stride(1) == F + 3 and (dense is None or dense.stride(1) == nd + 3)
    return ids, dense


def _single(c, s, B, err, hm=True, form=0, ids_wide=None, table=None, out=None):
    """Batch s's first B samples through rs_embed_fm_fwd_hm (or rs_embed_fm_fwd)
    under a kernel form, into a buffer with CANARY floats behind the logits
    (checked untouched)."""
    from recommender_system_amd import _lib
    ids, dense = _views(c, ids_wide)
    ids, dense = ids[s, :B], (dense[s, :B] if dense is not None else None)
    buf = torch.full((B + CANARY,), 99.0, device=ids.device) if out is None else out
    table = c["table"] if table is None else table
    head = [ids.data_ptr(), c["kind"], ids.stride(0), None if dense is None else dense.data_ptr(),
            0 if dense is None else dense.stride(0), c["nd"], table.data_ptr(), c["offs"].data_ptr(),
            c["voc"].data_ptr()]
    tail = [c["F"], c["k"], c["prep"].data_ptr(), c["w0"].data_ptr(), c["kfm"], buf.data_ptr(), None, B,
            err.data_ptr(), 0]
    prev = _lib.set_option(_lib.OPT_EMBED_FM_KERNEL, form)
    try:
        if hm:
            _lib.call("rs_embed_fm_fwd_hm", *head, C.addressof(c["hoff"]), C.addressof(c["hvoc"]), *tail)
        else:
            _lib.call("rs_embed_fm_fwd", *head, *tail)
    finally:
        _lib.set_option(_lib.OPT_EMBED_FM_KERNEL, prev)
    torch.cuda.synchronize()
    assert bool((buf[B:] == 99.0).all()), "floats behind the logits written"
    return buf[:B]


def _stream(c, B, err):
    """The S batches' first B samples in one streamed launch."""
    from recommender_system_amd import _lib
    ids, dense = _views(c)
    ids, dense = ids[:, :B], (dense[:, :B] if dense is not None else None)
    logit = torch.full((S, B), 77.0, device=ids.device)
    _lib.call("rs_embed_fm_fwd_hm_stream", ids.data_ptr(), c["kind"], ids.stride(1), ids.stride(0),
              None if dense is None else dense.data_ptr(), 0 if dense is None else dense.stride(1),
              0 if dense is None else dense.stride(0), c["nd"], c["table"].data_ptr(), C.addressof(c["hoff"]),
              C.addressof(c["hvoc"]), c["F"], c["k"], c["prep"].data_ptr(), c["w0"].data_ptr(), c["kfm"],
              logit.data_ptr(), logit.stride(0), B, S, B, 1, err.data_ptr(), 0)
    torch.cuda.synchronize()
    return logit


@pytest.mark.gpu
@pytest.mark.parametrize("idt", [torch.int32, torch.int64], ids=["i32", "i64"])
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("F,nd", SHAPES)
def test_ifetch_levers_bit_identical(gpu, F, nd, B, idt):
    from recommender_system_amd.layers import _ErrFlag
    c = _case(F, nd, idt)
    err = _ErrFlag(torch.device("cuda"))
    st = _stream(c, B, err.t)
    for s in range(S):  # batch 1: the two-pass waves' fields 0 / VOCAB - 1 (a swapped half shows)
        got = _single(c, s, B, err.t)
        assert torch.equal(got, _single(c, s, B, err.t, hm=False)), f"batch {s}: rs_embed_fm_fwd_hm vs rs_embed_fm_fwd"
        assert torch.equal(got, _single(c, s, B, err.t, form=4)), f"batch {s}: default vs struct-argument form"
        assert torch.equal(got, st[s]), f"batch {s}: the single launch vs the streamed one (S = 2)"
        assert_scaled_close(got, c["ref"][s, :B], what=f"batch {s}: rs_embed_fm_fwd_hm vs oracle")
    assert int(err.t.item()) == 0, "error word set by a clean run"


# Row length k and FM width kfm away from 16 / 10: KV = k / 4 floats per lane,
# NT = ceil((kfm + 1) / 16) column tiles.  The merged id load exists only where
# the body runs its two-pass schedule (KV * NT <= 8); k 64 and k 32 with two
# column tiles take the pass-at-a-time loop and must keep one id load per
# pass — with the merged load there, half the lanes of a two-pass wave would
# decode the other field's id and the second pass a stale one.
GEOMETRIES = [(64, 10), (32, 16), (32, 10), (16, 16), (8, 10), (4, 10)]  # (k, kfm)


@pytest.mark.gpu
@pytest.mark.parametrize("idt", [torch.int32, torch.int64], ids=["i32", "i64"])
@pytest.mark.parametrize("B", [17, 33])
@pytest.mark.parametrize("F", [17, 26, 32])
@pytest.mark.parametrize("k,kfm", GEOMETRIES)
def test_other_geometries_bit_identical(gpu, k, kfm, F, B, idt):
    """rs_embed_fm_fwd_hm == rs_embed_fm_fwd (device metadata, one id load per
    pass) == the struct-argument form, bit for bit, with one, ten and sixteen
    two-pass waves, on random ids and on the 0 / VOCAB - 1 batch; and the
    fp64 oracle.  Tolerance: the suite's 1e-5 stands for the headline's d =
    429 summed terms; the rounding error of an fp32 sum grows with the square
    root of their number, so it is scaled by sqrt(d / 429) where d is larger
    (2.2e-5 at k 64, 32 fields), never below 1e-5."""
    from recommender_system_amd.layers import _ErrFlag
    nd = 3
    c = _case(F, nd, idt, k, kfm)
    err = _ErrFlag(torch.device("cuda"))
    rtol = 1e-5 * max(1.0, ((nd + F * k) / 429.0) ** 0.5)
    for s in range(S):
        got = _single(c, s, B, err.t)
        assert torch.equal(got, _single(c, s, B, err.t, hm=False)), f"batch {s}: rs_embed_fm_fwd_hm vs rs_embed_fm_fwd"
        assert torch.equal(got, _single(c, s, B, err.t, form=4)), f"batch {s}: default vs struct-argument form"
        assert_scaled_close(got, c["ref"][s, :B], rtol=rtol, what=f"batch {s}: rs_embed_fm_fwd_hm vs oracle")
    assert int(err.t.item()) == 0, "error word set by a clean run"


@pytest.mark.gpu
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("F,nd", SHAPES)
def test_lds_garbage_never_reaches_a_logit(gpu, F, nd, B):
    """Two launches into one buffer; between them the same 1,024-thread kernel
    runs on a table of NaNs over every CU (512 tiles), so its partial tiles
    and q slots leave NaNs in LDS: the second launch's logits equal the
    first's bit for bit, and both are finite."""
    from recommender_system_amd.layers import _ErrFlag
    c = _case(F, nd, torch.int32)
    err = _ErrFlag(torch.device("cuda"))
    buf = torch.full((B + CANARY,), 99.0, device="cuda")
    first = _single(c, 0, B, err.t, out=buf).clone()
    nan_table = torch.full_like(c["table"], float("nan"))
    rep = lambda x: None if x is None else x[:1, :1].expand(1, 8192, x.shape[-1]).contiguous()
    big = {**c, "ids_wide": rep(c["ids_wide"]), "dense_wide": rep(c["dense_wide"])}
    poisoned = _single(big, 0, 8192, err.t, table=nan_table)
    assert bool(torch.isnan(poisoned).all()), "the poisoning launch did not produce NaNs"
    second = _single(c, 0, B, err.t, out=buf)
    assert bool(torch.isfinite(first).all()) and torch.equal(first, second)
    assert int(err.t.item()) == 0, "error word set by a clean run"


def _bad_columns(F):
    """(field of the first wave without a second pass, field of a two-pass
    wave's second pass); None where the shape has no such wave."""
    slack = None if F >= 32 else max(F - 16, 0)
    return slack, (F - 1 if F > 16 else None)


@pytest.mark.gpu
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("F,nd", SHAPES)
def test_bad_id_in_one_pass_and_two_pass_waves(gpu, F, nd, B):
    """An out-of-range id in the last sample of the last tile, in the first
    one-pass wave's field and, separately, in a two-pass wave's second field:
    IndexError both times, every other sample's logit as in the clean run."""
    from recommender_system_amd.layers import _ErrFlag
    c = _case(F, nd, torch.int32)
    err = _ErrFlag(torch.device("cuda"))
    clean = _single(c, 0, B, err.t)
    err.check("clean ids")
    for col, value in zip(_bad_columns(F), (VOCAB, -1)):
        if col is None:
            continue
        bad = c["ids_wide"].clone()
        bad[0, B - 1, 1 + col] = value
        got = _single(c, 0, B, err.t, ids_wide=bad)
        with pytest.raises(IndexError):
            err.check(f"bad id in field {col}")
        assert torch.equal(got[:B - 1], clean[:B - 1]), f"bad id in field {col}: other samples changed"
