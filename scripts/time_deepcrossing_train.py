"""Timing of DeepCrossing.train_step at the demo shape (26 fields, k 8, 13
dense, hidden [256, 256], 4 units; model/deepCrossing.py:36-45), B 4096:

  step_fused / step_composed : the whole step, fused=True against fused=False;
  fwd_fused                  : rs_deepcrossing_train_fwd (one launch) against
  fwd_composed               : the launches it replaces (rs_embed_gather,
                               rs_dense_fwd per layer, torch add / relu per
                               unit, the head's rs_dense_fwd);
  bwd_fused                  : rs_res_tower_bwd (one launch) against
  bwd_composed               : the data-path launches it replaces (the head's
                               and every layer's rs_gemm(trans_b) with its mask
                               epilogue, a torch mask and add per unit).

The weight gradients (rs_gemm(trans_a) + rs_col_sum per layer), the SGD update
and the embedding update are the same launches in both steps.  Each variant
is replayed from a captured graph (REPS calls per replay), the variants
alternate over ROUNDS rounds, times come from device events and the medians
are reported.  Prints one JSON line."""
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import recommender_system_amd as rs  # noqa: E402
from recommender_system_amd import _lib  # noqa: E402
from recommender_system_amd._lib import call, ptr  # noqa: E402

REPS = int(os.environ.get("DC_REPS", "10"))
ROUNDS = int(os.environ.get("DC_ROUNDS", "9"))


def runner(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        fn()
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            for _ in range(REPS):
                fn()
    torch.cuda.synchronize()
    return g.replay


def main():
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda")
    B, F, k, nd, hidden, U = int(os.environ.get("DC_B", "4096")), 26, 8, 13, [256, 256], 4
    rng = np.random.default_rng(0)
    vocabs = rng.integers(100, 100000, size=F)
    cols = [[{"feat": f"I{i + 1}"} for i in range(nd)],
            [{"feat": f"C{i + 1}", "feat_onehot_dim": int(v), "embed_dim": k} for i, v in enumerate(vocabs)]]
    make = lambda: rs.DeepCrossing(cols, 32, hidden, U, embed_dim=k, seed=0)
    mf, mc, m = make(), make(), make()
    ids = torch.as_tensor(np.stack([rng.integers(0, v, B) for v in vocabs], 1).astype(np.int32)).to(dev)
    dense = torch.rand(B, nd, device=dev)
    t = torch.as_tensor(rng.integers(0, 2, B).astype(np.float32)).to(dev)
    lr = 1e-4

    # the kernels alone, on fixed weights
    e, d, nh = m.embed_layer, m.d, len(hidden)
    ci = (C.c_int * nh)(*hidden)
    w = sum(hidden) + d
    emp = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
    saved, deltas, prob, logit, dx0, g = emp(B * (d + U * w)), emp(B * U * w), emp(B), emp(B), emp(B, d), emp(B)
    prep, prep_b, err = m.prepared(), m.prepared_bwd(), m._err.t
    units = [u._layers() for u in m.res_layer]
    head = m.output_layer
    gws = torch.empty(max(1, max(_lib.lib().rs_gemm_workspace_size(L.kernel.shape[0], L.kernel.shape[1], B)
                                 for L in m._all_layers())), dtype=torch.uint8, device=dev)
    gw = (ptr(gws), gws.numel())

    def fwd_fused():
        call("rs_deepcrossing_train_fwd", ptr(ids), _lib.id_kind(ids), ids.stride(0), ptr(dense), dense.stride(0), nd,
             ptr(e.table), ptr(e.field_offsets), ptr(e.field_vocab), F, k, nh, ci, U, ptr(prep), ptr(saved), ptr(prob),
             ptr(logit), B, ptr(err), _lib.stream())

    def fwd_composed():
        xs, acts = [e.gather(ids, dense, check_ids=False)], []
        for layers in units:
            au = [xs[-1]]
            for L in layers[:-1]:
                au.append(L(au[-1]))
            xs.append(torch.relu(xs[-1] + layers[-1](au[-1])))
            acts.append(au)
        z = emp(B)
        call("rs_dense_fwd", ptr(xs[-1]), d, ptr(head.kernel), ptr(head.bias), None, 0, ptr(z), 1, B, d, 1,
             _lib.stream())
        return xs, acts, z

    fwd_fused()
    xs0, acts0, z0 = fwd_composed()
    call("rs_head_grad", ptr(logit), ptr(logit), ptr(t), B, 1.0, 0.0, ptr(g), ptr(emp(B)), None, _lib.stream())

    def bwd_fused():
        call("rs_res_tower_bwd", ptr(saved), d, nh, ci, U, ptr(prep_b), None, 0, ptr(g), ptr(deltas), ptr(dx0), d, B,
             _lib.stream())

    def back(delta, L, a_in, masked):
        K_in, N_out = L.kernel.shape
        prev = emp(B, K_in)
        call("rs_gemm", 0, 1, B, K_in, N_out, 1.0, ptr(delta), delta.stride(0), ptr(L.kernel), N_out, 0.0, ptr(prev),
             K_in, ptr(a_in) if masked else None, a_in.stride(0), *gw, _lib.stream())
        return prev

    def bwd_composed():
        dy = back(g.view(B, 1), head, xs0[-1], False)
        for u in reversed(range(U)):
            eu = dy * (xs0[u + 1] > 0)
            delta = eu
            for li in reversed(range(nh + 1)):
                delta = back(delta, units[u][li], acts0[u][li], li > 0)
            dy = eu + delta
        return dy

    bwd_fused()
    dref = bwd_composed()
    torch.cuda.synchronize()
    # (the two forwards round differently: at this size a few of the 12 M ReLU
    # inputs change sign between them, and each flip moves its sample's row of
    # dx0 — so the share of elements that differ is reported beside the maximum)
    rel = (dx0 - dref).abs() / dref.abs().max()
    agree = {"logit": float((logit - z0).abs().max() / z0.abs().max()), "dx0": float(rel.max()),
             "dx0_share_beyond_1e-5": float((rel > 1e-5).float().mean())}

    parts = {
        "step_fused": lambda: mf.train_step((dense, ids), t, lr=lr, check_ids=False, fused=True),
        "step_composed": lambda: mc.train_step((dense, ids), t, lr=lr, check_ids=False, fused=False),
        "fwd_fused": fwd_fused, "fwd_composed": fwd_composed,
        "bwd_fused": bwd_fused, "bwd_composed": bwd_composed,
    }
    runners = {n: runner(fn) for n, fn in parts.items()}
    times = {n: [] for n in parts}
    names = list(parts)
    for r in range(ROUNDS):
        for n in (names if r % 2 == 0 else names[::-1]):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            runners[n]()
            e1.record()
            torch.cuda.synchronize()
            times[n].append(e0.elapsed_time(e1) * 1e3 / REPS)
    med = {n: float(np.median(v)) for n, v in times.items()}
    print(json.dumps({
        "workload": f"DeepCrossing.train_step F {F} k {k} nd {nd} hidden {hidden} units {U} B {B}",
        "median_us": {n: round(v, 2) for n, v in med.items()},
        "min_us": {n: round(float(np.min(v)), 2) for n, v in times.items()},
        "max_us": {n: round(float(np.max(v)), 2) for n, v in times.items()},
        "fused_over_composed": {p: round(med[p + "_fused"] / med[p + "_composed"], 3) for p in ("step", "fwd", "bwd")},
        "max_rel_diff_fused_vs_composed": agree, "reps": REPS, "rounds": ROUNDS}))


if __name__ == "__main__":
    main()
