"""The kernarg-metadata FM kernels with their hot arguments preloaded into
SGPRs (RS_OPT_EMBED_FM_KERNEL 5: embed_fm_mfma_kp / embed_fm_stream_kp)
against the struct-argument form (4), the default (0), rs_embed_fm_fwd and the
fp64 oracle.  The kernel body is shared, so every comparison between kernels
is bit for bit.

Shapes: the smallest at which the argument split can go wrong — B around the
16-sample tile (the clamp on the preloaded batch), the compile-time-geometry
shape (26 fields / 13 dense / FM width 10 / k 16) and three generic ones
(a wave with no field that owns a dense k-step, no dense block, one field),
int32 and int64 ids, and id / dense row strides wider than the rows (column
slices of wider tensors: the preloaded strides)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle import ctr_oracle as O
from tests.helpers import assert_scaled_close, random_ids

K, KFM, VOCAB = 16, 10, 50
S_MAX, B_MAX = 3, 33
SHAPES = [(26, 13), (9, 2), (32, 0), (1, 13)]  # (F, nd)
FORMS = {"default": 0, "struct": 4, "preload": 5}


def test_compile_time_geometry_and_fallback():
    """Host only: at 26 / 13 / 10 / 16 the launchers' compile-time geometry
    equals the packed image's (the specialised kernels run); every neighbouring
    shape takes the generic kernels; the two new option values are accepted."""
    from recommender_system_amd import _lib
    lib = _lib.lib()
    assert lib.rs_embed_fm_ct_geom(13, 26, 16, 10) == 1
    for nd, F, k, kfm in [(12, 26, 16, 10), (14, 26, 16, 10), (13, 25, 16, 10), (13, 27, 16, 10), (13, 26, 8, 10),
                          (13, 26, 32, 10), (13, 26, 16, 9), (13, 26, 16, 11), (13, 26, 6, 10), (-1, 26, 16, 10)]:
        assert lib.rs_embed_fm_ct_geom(nd, F, k, kfm) == 0, (nd, F, k, kfm)
    opt = _lib.OPT_EMBED_FM_KERNEL
    cur = lib.rs_get_option(opt)
    try:
        for v in (4, 5):
            assert lib.rs_set_option(opt, v) >= 0 and lib.rs_get_option(opt) == v
        assert lib.rs_set_option(opt, 6) == -1 and lib.rs_get_option(opt) == 5
    finally:
        lib.rs_set_option(opt, cur)


@functools.lru_cache(maxsize=None)
def _case(F, nd, idt):
    """One weight set, S_MAX x B_MAX samples and their fp64 logits per shape
    (computed once; the tests take leading samples of each batch)."""
    from recommender_system_amd import _lib
    dev = torch.device("cuda")
    rng = np.random.default_rng(1000 * F + nd)
    vocabs = [VOCAB] * F
    offs = np.arange(F, dtype=np.int64) * VOCAB
    d = nd + F * K
    table = rng.uniform(-0.05, 0.05, size=(F * VOCAB, K)).astype(np.float32)
    w1 = (rng.standard_normal((d, 1)) * 0.05).astype(np.float32)
    v = (rng.standard_normal((d, KFM)) * 0.05).astype(np.float32)
    w0 = np.array([0.017], np.float32)
    ids = np.stack([random_ids(rng, B_MAX, vocabs) for _ in range(S_MAX)])
    ids[0, 0] = VOCAB - 1
    dense = rng.random((S_MAX, B_MAX, nd)).astype(np.float32)
    tables = [table[o:o + VOCAB] for o in offs]
    ref = np.stack([O.fm_layer(np.concatenate([dense[s], O.embed_layer(ids[s], tables, np.float64)], 1),
                               w0, w1, v)[:, 0] for s in range(S_MAX)])
    t = lambda a, dt=torch.float32: torch.as_tensor(a).to(dt).to(dev).contiguous()
    c = {"F": F, "nd": nd, "ids_np": ids, "ref": ref, "kind": 0 if idt == torch.int32 else 1, "idt": idt,
         "table": t(table), "w0": t(w0), "offs": t(offs, torch.int64), "voc": t(vocabs, torch.int64),
         "hoff": (C.c_int64 * F)(*offs), "hvoc": (C.c_int64 * F)(*vocabs)}
    w1_d, v_d = t(w1), t(v)
    c["prep"] = torch.empty(_lib.lib().rs_fm_prepared_size(nd, F, K, KFM), device=dev)
    _lib.call("rs_fm_prepare", w1_d.data_ptr(), v_d.data_ptr(), nd, F, K, KFM, c["prep"].data_ptr(), 0)
    # rows wider than the data: ids in columns 2 .. 2+F of F+5, dense in 1 .. 1+nd of nd+3
    c["ids_wide"] = _wide(t(ids, idt), 2, 3, -7)
    c["dense_wide"] = _wide(t(dense), 1, 2, 99.0) if nd else None
    torch.cuda.synchronize()
    return c


def _wide(x, before, after, fill):
    w = torch.full(x.shape[:-1] + (before + x.shape[-1] + after,), fill, dtype=x.dtype, device=x.device)
    w[..., before:before + x.shape[-1]] = x
    return w


def _views(c, ids_wide=None):
    F, nd = c["F"], c["nd"]
    ids = (c["ids_wide"] if ids_wide is None else ids_wide)[:, :, 2:2 + F]
    dense = c["dense_wide"][:, :, 1:1 + nd] if nd else None
    return ids, dense


class _Form:
    def __init__(self, value):
        self.value = value

    def __enter__(self):
        from recommender_system_amd import _lib
        self.prev = _lib.set_option(_lib.OPT_EMBED_FM_KERNEL, self.value)

    def __exit__(self, *exc):
        from recommender_system_amd import _lib
        _lib.set_option(_lib.OPT_EMBED_FM_KERNEL, self.prev)


def _single(c, s, B, form, err, hm=True, ids_wide=None):
    """One batch through rs_embed_fm_fwd_hm (or rs_embed_fm_fwd) under a kernel form."""
    from recommender_system_amd import _lib
    ids, dense = _views(c, ids_wide)
    ids, dense = ids[s, :B], (dense[s, :B] if dense is not None else None)
    assert ids.stride(0) > c["F"] and (dense is None or dense.stride(0) > c["nd"])
    logit = torch.full((B,), 99.0, device=ids.device)
    head = [ids.data_ptr(), c["kind"], ids.stride(0), None if dense is None else dense.data_ptr(),
            0 if dense is None else dense.stride(0), c["nd"], c["table"].data_ptr(), c["offs"].data_ptr(),
            c["voc"].data_ptr()]
    tail = [c["F"], K, c["prep"].data_ptr(), c["w0"].data_ptr(), KFM, logit.data_ptr(), None, B, err.data_ptr(), 0]
    with _Form(FORMS[form]):
        if hm:
            _lib.call("rs_embed_fm_fwd_hm", *head, C.addressof(c["hoff"]), C.addressof(c["hvoc"]), *tail)
        else:
            _lib.call("rs_embed_fm_fwd", *head, *tail)
    torch.cuda.synchronize()
    return logit


def _stream(c, S, B, last, form, err, ids_wide=None):
    from recommender_system_amd import _lib
    ids, dense = _views(c, ids_wide)
    ids, dense = ids[:S, :B], (dense[:S, :B] if dense is not None else None)
    logit = torch.full((S, B), 77.0, device=ids.device)
    with _Form(FORMS[form]):
        _lib.call("rs_embed_fm_fwd_hm_stream", ids.data_ptr(), c["kind"], ids.stride(1), ids.stride(0),
                  None if dense is None else dense.data_ptr(), 0 if dense is None else dense.stride(1),
                  0 if dense is None else dense.stride(0), c["nd"], c["table"].data_ptr(), C.addressof(c["hoff"]),
                  C.addressof(c["hvoc"]), c["F"], K, c["prep"].data_ptr(), c["w0"].data_ptr(), KFM, logit.data_ptr(),
                  logit.stride(0), B, S, last, 1, err.data_ptr(), 0)
    torch.cuda.synchronize()
    return logit


@pytest.mark.gpu
@pytest.mark.parametrize("idt", [torch.int32, torch.int64], ids=["i32", "i64"])
@pytest.mark.parametrize("B", [1, 15, 16, 17, 33])
@pytest.mark.parametrize("F,nd", SHAPES)
def test_preloaded_form_bit_identical(gpu, F, nd, B, idt):
    from recommender_system_amd.layers import _ErrFlag
    c = _case(F, nd, idt)
    err = _ErrFlag(torch.device("cuda"))
    got = _single(c, 0, B, "preload", err.t)
    assert torch.equal(got, _single(c, 0, B, "struct", err.t)), "preloaded vs struct-argument form"
    assert torch.equal(got, _single(c, 0, B, "default", err.t)), "preloaded form vs the default"
    assert torch.equal(got, _single(c, 0, B, "preload", err.t, hm=False)), "preloaded form vs rs_embed_fm_fwd"
    assert_scaled_close(got, c["ref"][0, :B], what="preloaded form vs oracle")
    err.check("clean ids")

    last = min(5, B)  # the ragged last batch
    for S in (1, 3):
        st = _stream(c, S, B, last, "preload", err.t)
        assert torch.equal(st, _stream(c, S, B, last, "struct", err.t)), f"stream S={S}: preloaded vs struct form"
        for s in range(S):
            n = B if s < S - 1 else last
            assert torch.equal(st[s, :n], _single(c, s, n, "preload", err.t)), f"stream S={S} batch {s}"
            assert_scaled_close(st[s, :n], c["ref"][s, :n], what=f"stream S={S} batch {s} vs oracle")
        assert bool((st[S - 1, last:] == 77.0).all()), "rows past the last batch's length written"
    err.check("clean ids (stream)")

    # a bad id in the last sample's last field: the (cold) err pointer
    bad = c["ids_wide"].clone()
    bad[0, B - 1, 2 + F - 1] = VOCAB
    _single(c, 0, B, "preload", err.t, ids_wide=bad)
    with pytest.raises(IndexError):
        err.check("bad id")
    bad = c["ids_wide"].clone()
    bad[0, last - 1, 2 + F - 1] = VOCAB
    _stream(c, 1, B, last, "preload", err.t, ids_wide=bad)
    with pytest.raises(IndexError):
        err.check("bad id (stream)")
