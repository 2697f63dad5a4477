"""Fingerprint of every training step: which entry points a step issues, with
which scalar arguments, and the bits it leaves behind.

For each case and each of B = 33 (below one 64-row K slice: rs_gemm cannot
split) and B = 200 (it splits) the model is built from a fixed seed, three
``train_step``s run on fixed random inputs, and one JSON line is written:

  launch_table : the distinct [name, arg, ...] records of the librs_hip entry
             points the three steps called through ``_lib.call`` — the
             arguments whose ctypes type is not a pointer (ints and floats),
             and the elements of int / float arrays; pointers and the stream
             are left out — in order of first use
  launches : the ordered list of calls, each an index into launch_table (a
             step repeats most records, so the table keeps the line short
             and loses nothing)
  weights  : SHA-256 of every tensor in ``keras_weights()`` after the steps
             (and of the table shard of the sharded models)
  losses   : SHA-256 of the three returned loss vectors
  dropout_offset : the dropout generator's offset (None where none was made)

Sizes: 3 sparse fields with vocabularies 5, 7 and 11, two dense features,
k = 8, hidden units [32, 16], T = 4 for DIN.  Two outputs of one tree tell
which cases are reproducible in themselves; outputs of two trees tell whether
a host-side change kept the launches and the bits.  The script uses only the
public model classes and ``models._dropout_rng``; it records launches by
replacing the name ``call`` in every loaded module of the package that has
one, so it runs unchanged on trees that place their helpers differently.

  python scripts/train_fingerprint.py OUT.jsonl [case-name-prefix ...]
"""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import recommender_system_amd as rs  # noqa: E402
from recommender_system_amd import _lib, models as M  # noqa: E402
from recommender_system_amd import sharded as S  # noqa: E402

VOCABS, ND, K, HIDDEN, T, STEPS = [5, 7, 11], 2, 8, [32, 16], 4, 3
BATCHES = (33, 200)
_SCALARS = (C.c_int, C.c_int64, C.c_float, C.c_double, C.c_uint64, C.c_uint32)

_launches = []
_real_call = _lib.call


def _recording_call(name, *args):
    types = _lib.SIGNATURES[name][1]
    rec = [name]
    for a, t in zip(args, types):
        if isinstance(a, C.Array):
            if a._type_ in _SCALARS:
                rec.append([v for v in a])
        elif t is not C.c_void_p and isinstance(a, (int, float)):
            rec.append(a)
    _launches.append(rec)
    _real_call(name, *args)


def _wrap_calls():
    for name, mod in list(sys.modules.items()):
        if name.startswith("recommender_system_amd") and mod is not None and getattr(mod, "call", None) is _real_call:
            mod.call = _recording_call


def _sha(t):
    a = t.detach().cpu().contiguous().numpy()
    return hashlib.sha256(a.tobytes()).hexdigest()


def _columns():
    return [[{"feat": f"I{i + 1}"} for i in range(ND)],
            [{"feat": f"C{i + 1}", "feat_onehot_dim": v, "embed_dim": K} for i, v in enumerate(VOCABS)]]


def _criteo_batch(rng, B):
    dense = rng.random((B, ND)).astype(np.float32)
    ids = np.stack([rng.integers(0, v, B) for v in VOCABS], 1).astype(np.int32)
    return dense, ids, rng.integers(0, 2, B).astype(np.float32)


def _criteo_case(make, **kw):
    def run(rng, B):
        m = make()
        losses = []
        for _ in range(STEPS):
            dense, ids, t = _criteo_batch(rng, B)
            losses.append(m.train_step((dense, ids), t, lr=0.1, return_loss=True, **kw))
        return m, losses
    return run


def _fm_case(rng, B):
    m = rs.FM(K, 1e-3, 2e-3, seed=3)
    offs = np.concatenate([[0], np.cumsum(VOCABS)[:-1]])
    losses = []
    for _ in range(STEPS):
        dense, ids, t = _criteo_batch(rng, B)
        losses.append(m.train_step(dense, ids, t, offs, np.array(VOCABS), lr=0.1, return_loss=True))
    return m, losses


def _din_case(att, dnn, fused):
    def run(rng, B):
        cols = [[{"feat": "price"}],
                [{"feat": "user_id", "feat_onehot_dim": 11, "embed_dim": K},
                 {"feat": "movie_seq", "feat_onehot_dim": 7, "embed_dim": K},
                 {"feat": "cate_seq", "feat_onehot_dim": 5, "embed_dim": K}]]
        beh = ["movie_seq", "cate_seq"]
        m = rs.DIN(cols, beh, att_hidden_units=(32, 16), dnn_hidden_units=tuple(HIDDEN), att_attention=att,
                   dnn_activation=dnn, dnn_dropout=0.2, seed=3)
        m.fused_att_train = fused
        losses = []
        for _ in range(STEPS):
            lens = rng.integers(0, T + 1, size=B)
            valid = np.arange(T)[None, :] < lens[:, None]
            inputs = {"user_id": rng.integers(0, 11, (B, 1)).astype(np.int64),
                      "movie_seq": np.where(valid, rng.integers(1, 7, (B, T)), 0).astype(np.int64),
                      "cate_seq": np.where(valid, rng.integers(1, 5, (B, T)), 0).astype(np.int64),
                      "price": rng.random((B, 1)).astype(np.float32),
                      "movie_id": np.stack([rng.integers(0, 7, B), rng.integers(0, 5, B)], 1).astype(np.int64)}
            t = rng.integers(0, 2, B).astype(np.float32)
            losses.append(m.train_step(inputs, t, lr=0.1, return_loss=True))
        return m, losses
    return run


def _widedeep_case(onehot):
    def run(rng, B):
        m = rs.WideDeep(_columns(), HIDDEN, 1, "relu", embed_dim=K, seed=3, w_reg=1e-3)
        widths = np.array(VOCABS, np.int64)
        offs = np.concatenate([[0], np.cumsum(widths)[:-1]])
        m.build(2 * ND + int(widths.sum()))
        losses = []
        for _ in range(STEPS):
            dense, ids, t = _criteo_batch(rng, B)
            if onehot:
                losses.append(m.train_step_onehot(dense, ids, offs, widths, t, lr=0.1, return_loss=True))
            else:
                dummies = np.zeros((B, int(widths.sum())), np.float32)
                dummies[np.arange(B)[:, None], offs[None, :] + ids] = 1.0
                X = np.concatenate([dense, ids.astype(np.float32), dense, dummies], 1)
                losses.append(m.train_step(X, t, lr=0.1, return_loss=True))
        return m, losses
    return run


def _sharded_fm_case(rng, B):
    m = S.ShardedEmbeddingFM(VOCABS, K, ND, 4, device="cuda", seed=3, world=1, rank=0)
    losses = []
    for _ in range(STEPS):
        dense, ids, t = _criteo_batch(rng, B)
        dev = lambda a: torch.as_tensor(a, device="cuda")
        losses.append(m.train_step(dev(dense), dev(ids), dev(t), lr=0.1, return_loss=True))
    return m, losses


def _sharded_deepfm_case(rng, B):
    m = S.ShardedDeepFM(_columns(), 4, 1e-3, 2e-3, HIDDEN, 1, "relu", embed_dim=K, device="cuda", seed=3, world=1,
                        rank=0)
    losses = []
    for _ in range(STEPS):
        dense, ids, t = _criteo_batch(rng, B)
        losses.append(m.train_step((dense, ids), t, lr=0.1, return_loss=True, dropout=0.2))
    return m, losses


def _cases():
    cols = _columns
    deepfm = lambda: rs.DeepFM(cols(), 4, 1e-3, 2e-3, HIDDEN, 1, "relu", embed_dim=K, seed=3)
    dcn = lambda n: (lambda: rs.DCN(cols(), HIDDEN, 4, "relu", n, embed_dim=K, seed=3))
    pnn = lambda mode: (lambda: rs.PNN(cols(), mode, HIDDEN, 1, embed_dim=K, seed=3))
    deepx = lambda: rs.DeepCrossing(cols(), 8, HIDDEN, 2, embed_dim=K, seed=3)
    return {
        "fm": _fm_case,
        "deepfm_dropout": _criteo_case(deepfm, dropout=0.2),
        "deepfm_nodrop": _criteo_case(deepfm, dropout=False),
        "dcn_cross2": _criteo_case(dcn(2), dropout=0.2),
        "dcn_cross0": _criteo_case(dcn(0), dropout=0.2),
        "pnn_inner": _criteo_case(pnn("inner")),
        "pnn_outer": _criteo_case(pnn("outer")),
        "pnn_both": _criteo_case(pnn("both")),
        "nfm_dropout": _criteo_case(lambda: rs.NFM(cols(), HIDDEN, 4, "relu", 0.2, embed_dim=K, seed=3)),
        "ffm": _criteo_case(lambda: rs.FFM(cols(), 4, w_reg=1e-3, v_reg=2e-3, seed=3)),
        "din_prelu_fused": _din_case("prelu", "prelu", True),
        "din_prelu_unfused": _din_case("prelu", "prelu", False),
        "din_dice": _din_case("dice", "dice", True),
        "deepcrossing_fused": _criteo_case(deepx, fused=True),
        "deepcrossing_composed": _criteo_case(deepx, fused=False),
        "widedeep_packed": _widedeep_case(False),
        "widedeep_onehot": _widedeep_case(True),
        "sharded_fm": _sharded_fm_case,
        "sharded_deepfm_dropout": _sharded_deepfm_case,
    }


def _indexed(launches):
    """(distinct records in order of first use, the calls as indices into them)."""
    table, seen, order = [], {}, []
    for rec in launches:
        key = json.dumps(rec)
        if key not in seen:
            seen[key] = len(table)
            table.append(rec)
        order.append(seen[key])
    return table, order


def _weights(m):
    if isinstance(m, S.ShardedEmbeddingFM):
        w = {"w0": m.w0, "w1": m.w1, "v": m.v, "table_shard": m.table_shard}
    else:
        w = dict(m.keras_weights())
        if isinstance(m, S.ShardedDeepFM):
            w["table_shard"] = m.table_shard
    return {n: _sha(t) for n, t in sorted(w.items())}


def _dropout_offset(m):
    if isinstance(m, S.ShardedDeepFM):
        rng = m._drop_rng  # seeded per rank, kept by the model itself
    else:
        rng = M._dropout_rng(m) if "_drop_rng" in m.__dict__ else None
    return None if rng is None else rng.offset


def main():
    assert torch.cuda.is_available(), "needs an MI355X"
    out, only = sys.argv[1], sys.argv[2:]
    _wrap_calls()
    with open(out, "w") as f:
        for name, run in _cases().items():
            if only and not any(name.startswith(p) for p in only):
                continue
            for B in BATCHES:
                del _launches[:]
                torch.manual_seed(0)
                try:
                    m, losses = run(np.random.default_rng(1000 + B), B)
                except (ValueError, NotImplementedError, TypeError, KeyError, AttributeError) as e:
                    # a host-side refusal of the case's arguments (never a device error): recorded, not hidden
                    f.write(json.dumps({"case": name, "B": B, "error": f"{type(e).__name__}: {e}"}) + "\n")
                    print(f"{name} B={B}: {type(e).__name__}: {e}", flush=True)
                    continue
                torch.cuda.synchronize()
                table, order = _indexed(_launches)
                line = {"case": name, "B": B, "launch_table": table, "launches": order, "weights": _weights(m),
                        "losses": [_sha(l) for l in losses], "dropout_offset": _dropout_offset(m)}
                f.write(json.dumps(line, separators=(",", ":")) + "\n")
                f.flush()
                print(f"{name} B={B}: {len(_launches)} launches", flush=True)


if __name__ == "__main__":
    main()
