"""Timing of FNN (model/fnn.py) on the compact batch: nd 13, k 8, DNN
[256, 128, 64] -> 1, at B 32 and B 4096, on two vocabularies:

  full    : the 26 field widths of tests/golden/criteo_ref.npz (n = 13 + 43 605
            one-hot columns).  The reference's dense form is not run here: its
            sizes are the result (``dense_form_bytes``).
  reduced : every field capped at 64 codes, where the dense form fits and a
            plain torch restatement of it on the same GPU is the baseline.

Per shape (median of ROUNDS rounds of REPS back-to-back calls, device events,
the variants alternating; microseconds per call):

  project        rs_fnn_project (once per weight set)      + achieved GB/s
  gather         rs_fnn_first_layer_fwd alone              + achieved GB/s
  fwd_fused      rs_fnn_fwd (one launch)
  fwd_composed   rs_fnn_first_layer_fwd + rs_mlp_fwd
  train_fwd      rs_fnn_train_fwd (sort + Pu + z1)
  w1_sgd         rs_fnn_w1_sgd (lr 0: the weights stay put)
  step           FNN.train_step (dropout 0.2, check_ids=False), host included
  fwd_torch      the dense tower on a prebuilt x (.) v [B, n*k] (reduced only)
  fwd_torch_xv   the same with (X[:, :, None] * v).reshape(B, n*k) inside
  step_torch     torch autograd + SGD on the prebuilt x (.) v, dropout 0.2

The GB/s figures divide the bytes the kernel must move (computed from the
shapes: rows read + rows written + ids) by its time; they are rates of
whatever level of the memory hierarchy serves the rows, not HBM rates.
Writes one JSON line per shape to --out (default profiles/fnn_timing.jsonl)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import recommender_system_amd as rs  # noqa: E402
from recommender_system_amd import _lib  # noqa: E402
from recommender_system_amd._lib import call, ints, ptr  # noqa: E402

REPS = int(os.environ.get("FNN_REPS", "20"))
ROUNDS = int(os.environ.get("FNN_ROUNDS", "7"))
ND, K, HIDDEN = 13, 8, [256, 128, 64]


def measure(parts):
    for fn in parts.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times, order = {nm: [] for nm in parts}, list(parts)
    for r in range(ROUNDS):
        for nm in (order if r % 2 == 0 else order[::-1]):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(REPS):
                parts[nm]()
            e1.record()
            torch.cuda.synchronize()
            times[nm].append(e0.elapsed_time(e1) * 1e3 / REPS)
    return times


def shape(name, vocab, B, dev, with_torch):
    rng = np.random.default_rng(0)
    F, n = len(vocab), ND + int(sum(vocab))
    offs = np.concatenate([[0], np.cumsum(vocab)[:-1]]).astype(np.int64)
    m = rs.FNN(K, HIDDEN, device=dev, seed=0)
    m.build(n)
    dense = torch.as_tensor(rng.random((B, ND)).astype(np.float32)).to(dev)
    ids_h = np.stack([rng.integers(0, v, B) for v in vocab], 1).astype(np.int32)
    ids = torch.as_tensor(ids_h).to(dev)
    y = torch.as_tensor(rng.integers(0, 2, B).astype(np.float32)).to(dev)
    doffs, dvoc = torch.as_tensor(offs).to(dev), torch.as_tensor(np.asarray(vocab, np.int64)).to(dev)
    ls = m.dnn._layers()
    first, v = ls[0], m.fm.fm.v
    H1, st = first.units, _lib.stream
    dims, acts = ints([l.units for l in ls]), ints([_lib.ACT[l.activation] for l in ls])
    assert m.fused_ok()
    P, prep = m.projected(), m._rest.prepared()
    emp = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
    a1, yf, err = emp(B, H1), emp(B, 1), torch.zeros(1, dtype=torch.int32, device=dev)
    idk = _lib.id_kind(ids)

    def project():
        call("rs_fnn_project", ptr(v), ptr(first.kernel), n, K, H1, ptr(P), st())

    def gather():
        call("rs_fnn_first_layer_fwd", ptr(ids), idk, ids.stride(0), ptr(dense), ND, ND, ptr(doffs), ptr(dvoc), F,
             ptr(P), n, H1, ptr(first.bias), _lib.ACT[first.activation], ptr(a1), H1, B, ptr(err), st())

    def fwd_fused():
        call("rs_fnn_fwd", ptr(ids), idk, ids.stride(0), ptr(dense), ND, ND, ptr(doffs), ptr(dvoc), F, ptr(P), n,
             ptr(first.bias), len(ls), dims, acts, ptr(prep), ptr(yf), 1, B, ptr(err), st())

    def fwd_composed():
        gather()
        return m._rest.tower(a1, head=True)

    ws = torch.empty(_lib.lib().rs_fnn_train_workspace_size(B, ND, F, n, H1), dtype=torch.uint8, device=dev)
    d_a1, dz1 = torch.as_tensor(rng.normal(0, 1e-3, (B, H1)).astype(np.float32)).to(dev), emp(B, H1)

    def train_fwd():
        call("rs_fnn_train_fwd", ptr(ids), idk, ids.stride(0), ptr(dense), ND, ND, ptr(doffs), ptr(dvoc), F, ptr(v),
             ptr(first.kernel), n, K, H1, ptr(first.bias), 1, ptr(a1), H1, B, ptr(ws), ptr(err), st())

    def w1_sgd():
        call("rs_fnn_w1_sgd", ptr(d_a1), H1, None, 0, ptr(a1), H1, ptr(dense), ND, ND, F, ptr(v), ptr(first.kernel), n,
             K, H1, B, 0.0, ptr(dz1), None, ptr(ws), st())

    def step():
        m.train_step(dense, ids, y, offs, vocab, lr=1e-4, check_ids=False)

    parts = {"project": project, "gather": gather, "fwd_fused": fwd_fused, "fwd_composed": fwd_composed,
             "train_fwd": train_fwd, "w1_sgd": w1_sgd, "step": step}
    fwd_fused()
    agree = {"fused_vs_composed": float((yf - fwd_composed()).abs().max())}
    if with_torch:
        X = torch.zeros(B, n, device=dev)
        X[:, :ND] = dense
        X.scatter_(1, (ND + doffs + ids.long()), 1.0)
        xv = (X[:, :, None] * v).reshape(B, n * K)
        tp = [p.detach().clone().requires_grad_(True) for l in ls for p in (l.kernel, l.bias)]

        def tower(h, train):
            for i in range(len(ls) - 1):
                h = torch.relu(torch.nn.functional.linear(h, tp[2 * i].t(), tp[2 * i + 1]))
                if train:
                    h = torch.nn.functional.dropout(h, 0.2)
            return torch.nn.functional.linear(h, tp[-2].t(), tp[-1])

        def fwd_torch():
            with torch.no_grad():
                return torch.sigmoid(tower(xv, False))

        def fwd_torch_xv():
            with torch.no_grad():
                return torch.sigmoid(tower((X[:, :, None] * v).reshape(B, n * K), False))

        def step_torch():
            loss = torch.nn.functional.binary_cross_entropy_with_logits(tower(xv, True)[:, 0], y)
            grads = torch.autograd.grad(loss, tp)
            with torch.no_grad():
                for p, g in zip(tp, grads):
                    p.sub_(1e-4 * g)

        agree["fused_vs_torch"] = float((yf - fwd_torch()).abs().max())
        parts.update({"fwd_torch": fwd_torch, "fwd_torch_xv": fwd_torch_xv, "step_torch": step_torch})
    times = measure(parts)
    med = {nm: float(np.median(t)) for nm, t in times.items()}
    A = ND + F
    gather_bytes = B * A * H1 * 4 + B * H1 * 4 + B * F * 4 + B * ND * 4
    project_bytes = n * K * H1 * 4 + n * H1 * 4 + n * K * 4
    out = {"workload": f"FNN {name} vocabulary: nd {ND} F {F} n {n} k {K} DNN {HIDDEN}->1 B {B}",
           "median_us": {nm: round(x, 2) for nm, x in med.items()},
           "min_us": {nm: round(float(np.min(t)), 2) for nm, t in times.items()},
           "max_us": {nm: round(float(np.max(t)), 2) for nm, t in times.items()},
           "fused_over_composed": round(med["fwd_fused"] / med["fwd_composed"], 3),
           "gather_bytes": gather_bytes, "gather_GBps": round(gather_bytes / med["gather"] / 1e3, 1),
           "project_bytes": project_bytes, "project_GBps": round(project_bytes / med["project"] / 1e3, 1),
           "dense_form_bytes": {"input_B_nk": B * n * K * 4, "W1": n * K * H1 * 4, "P": n * H1 * 4},
           "max_abs_diff": agree, "reps": REPS, "rounds": ROUNDS}
    if with_torch:
        out["fused_over_torch"] = round(med["fwd_fused"] / med["fwd_torch"], 3)
        out["step_over_torch"] = round(med["step"] / med["step_torch"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fnn_timing.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda")
    full = [int(x) for x in np.load(os.path.join(ROOT, "tests", "golden", "criteo_ref.npz"))["vocab"]]
    reduced = [min(x, 64) for x in full]
    with open(args.out, "w") as f:
        for name, vocab, with_torch in (("reduced", reduced, True), ("full", full, False)):
            for B in (32, 4096):
                line = json.dumps(shape(name, vocab, B, dev, with_torch))
                print(line, flush=True)
                f.write(line + "\n")
                f.flush()


if __name__ == "__main__":
    main()
