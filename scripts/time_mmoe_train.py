"""Timing of MMOE.train_step at the timing shape of scripts/time_mmoe.py (d 221,
H 64, E 8, T 2, towers [32, 16], output 1), B 4096:

  step_fused / step_composed : the whole step, fused=True against fused=False;
  fwd_fused                  : rs_mmoe_train_fwd (one launch) against
  fwd_composed               : the launches it replaces (rs_dense_fwd for the
                               experts and per gate, torch softmax / multiply /
                               sum per task, rs_dense_fwd per tower layer);
  bwd_fused                  : rs_mmoe_bwd with dx (one launch) against
  bwd_composed               : the data-path launches it replaces (every tower
                               layer's rs_gemm(trans_b) with its mask epilogue,
                               the torch backward of the mix and the softmax,
                               the T + 1 rs_gemm(trans_b) of dx and their adds);
  step_torch                 : a plain fp32 torch-autograd step of the same
                               model and loss (torch.autograd.grad, then w -=
                               lr (g + 2 l2 w) per tensor) — the outside
                               yardstick.

The head, the weight gradients (rs_gemm(trans_a) + rs_col_sum per tensor) and
the SGD update are the same launches in both of the package's steps.  Each
variant is replayed from a captured graph (REPS calls per replay), the variants
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

REPS = int(os.environ.get("MMOE_REPS", "10"))
ROUNDS = int(os.environ.get("MMOE_ROUNDS", "9"))


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
    B, d, H, E, T, towers, nout = int(os.environ.get("MMOE_B", "4096")), 221, 64, 8, 2, [32, 16], 1
    rng = np.random.default_rng(0)
    make = lambda: rs.MMOE(H, E, T, towers, nout, device=dev, seed=0, input_dim=d)
    mf, mc, m = make(), make(), make()
    x = torch.as_tensor(rng.normal(0, 1, (B, d)).astype(np.float32)).to(dev)
    y = torch.as_tensor(rng.integers(0, 2, (T, B, nout)).astype(np.float32)).to(dev)
    lr, st = 1e-4, _lib.stream
    assert mf.train_fused_ok()

    # the kernels alone, on fixed weights
    ml, tw = m.mmoe_layer, [t._layers() for t in m.tower_layer]
    dims = [H] + towers + [nout]
    n, HE, N1 = len(dims) - 1, H * E, (H + T) * E
    ci, ca = (C.c_int * (n + 1))(*dims), (C.c_int * n)(*([1] * (n - 1) + [0]))
    emp = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
    saved = emp(_lib.lib().rs_mmoe_saved_size(d, H, E, T, n, ci, B))
    z, deltas, dz1, dx = emp(T, B, nout), emp(B * T * sum(towers)), emp(B, N1), emp(B, d)
    prep, prep_b = m.prepared(), m.prepared_bwd()

    def fwd_fused():
        call("rs_mmoe_train_fwd", ptr(x), d, d, H, E, T, n, ci, ca, ptr(prep), ptr(saved), ptr(z), B * nout, nout, B,
             st())

    def dense(a, kernel, bias, act):
        K, N = kernel.shape[0], kernel.numel() // kernel.shape[0]
        out = emp(a.shape[0], N)
        call("rs_dense_fwd", ptr(a), a.stride(0), ptr(kernel), ptr(bias), None, act, ptr(out), N, a.shape[0], K, N, st())
        return out

    def fwd_composed():
        exp3 = dense(x, ml.expert_matrix, ml.expert_bias, 1).view(B, H, E)
        ps, acts, zs = [], [], []
        for t in range(T):
            ps.append(torch.softmax(dense(x, ml.gate_matrix[t], ml.gate_bias[t], 0), dim=-1))
            a = [(exp3 * ps[t].unsqueeze(1)).sum(-1)]
            for L in tw[t][:-1]:
                a.append(dense(a[-1], L.kernel, L.bias, 1))
            zs.append(dense(a[-1], tw[t][-1].kernel, tw[t][-1].bias, 0))
            acts.append(a)
        return exp3, ps, acts, zs

    fwd_fused()
    exp3, ps, acts0, zs0 = fwd_composed()
    G = emp(B, T * nout)
    call("rs_mmoe_head_grad", ptr(z), B * nout, nout, ptr(y), B * nout, nout, None, nout, T, B, ptr(G), T * nout, None,
         st())

    def bwd_fused():
        call("rs_mmoe_bwd", ptr(saved), ptr(G), T * nout, d, H, E, T, n, ci, ca, ptr(prep_b), ptr(deltas), ptr(dz1), N1,
             ptr(dx), d, B, st())

    def back(delta, kernel, mask):
        K_in, N_out = kernel.shape[0], kernel.numel() // kernel.shape[0]
        prev = emp(B, K_in)
        call("rs_gemm", 0, 1, B, K_in, N_out, 1.0, ptr(delta), delta.stride(0), ptr(kernel), N_out, 0.0, ptr(prev), K_in,
             ptr(mask), 0 if mask is None else mask.stride(0), None, 0, st())
        return prev

    def bwd_composed():
        dexp, dlog = torch.zeros_like(exp3), []
        for t in range(T):
            delta = G[:, t * nout:(t + 1) * nout]
            for li in reversed(range(n)):
                delta = back(delta, tw[t][li].kernel, acts0[t][li] if li > 0 else None)
            dexp = dexp + delta.unsqueeze(2) * ps[t].unsqueeze(1)
            dp = (delta.unsqueeze(2) * exp3).sum(1)
            dlog.append(ps[t] * (dp - (ps[t] * dp).sum(-1, keepdim=True)))
        dz = torch.cat([(dexp * (exp3 > 0)).reshape(B, HE)] + dlog, 1)
        out = back(dz[:, :HE], ml.expert_matrix, None)
        for t in range(T):
            out = out + back(dz[:, HE + t * E:HE + (t + 1) * E], ml.gate_matrix[t], None)
        return dz, out

    bwd_fused()
    dz_ref, dx_ref = bwd_composed()
    torch.cuda.synchronize()
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())
    agree = {"z": rel(z, torch.stack(zs0)), "dz1": rel(dz1, dz_ref), "dx": rel(dx, dx_ref)}

    # the outside yardstick: the same model, loss and update in plain torch autograd
    names = list(m.keras_weights())
    tp = [p.detach().clone().requires_grad_(True) for p in m.keras_weights().values()]
    l2s = [1e-4 if k.startswith("mmoe_layer/") else 0.0 for k in names]

    def step_torch():
        w = dict(zip(names, tp))
        ex = torch.relu(x @ w["mmoe_layer/expert_matrix"].view(d, HE) + w["mmoe_layer/expert_bias"].view(-1)).view(B, H, E)
        loss = 0.0
        for t in range(T):
            p = torch.softmax(x @ w[f"mmoe_layer/gate_matrix{t}"] + w[f"mmoe_layer/gate_bias{t}"], dim=-1)
            a = (ex * p.unsqueeze(1)).sum(-1)
            for i in range(n - 1):
                a = torch.relu(a @ w[f"tower_layer_{t}/dense_{i}/kernel"] + w[f"tower_layer_{t}/dense_{i}/bias"])
            zt = a @ w[f"tower_layer_{t}/dense_out/kernel"] + w[f"tower_layer_{t}/dense_out/bias"]
            loss = loss + torch.nn.functional.binary_cross_entropy_with_logits(zt, y[t])
        grads = torch.autograd.grad(loss, tp)
        with torch.no_grad():
            for p, g, l2 in zip(tp, grads, l2s):
                p.sub_(lr * (g + 2 * l2 * p))

    parts = {
        "step_fused": lambda: mf.train_step(x, y, lr=lr, fused=True),
        "step_composed": lambda: mc.train_step(x, y, lr=lr, fused=False),
        "fwd_fused": fwd_fused, "fwd_composed": fwd_composed,
        "bwd_fused": bwd_fused, "bwd_composed": bwd_composed,
        "step_torch": step_torch,
    }
    runners = {nm: runner(fn) for nm, fn in parts.items()}
    times = {nm: [] for nm in parts}
    order = list(parts)
    for r in range(ROUNDS):
        for nm in (order if r % 2 == 0 else order[::-1]):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            runners[nm]()
            e1.record()
            torch.cuda.synchronize()
            times[nm].append(e0.elapsed_time(e1) * 1e3 / REPS)
    med = {nm: float(np.median(v)) for nm, v in times.items()}
    print(json.dumps({
        "workload": f"MMOE.train_step d {d} H {H} E {E} T {T} towers {towers} out {nout} B {B}",
        "median_us": {nm: round(v, 2) for nm, v in med.items()},
        "min_us": {nm: round(float(np.min(v)), 2) for nm, v in times.items()},
        "max_us": {nm: round(float(np.max(v)), 2) for nm, v in times.items()},
        "fused_over_composed": {p: round(med[p + "_fused"] / med[p + "_composed"], 3) for p in ("step", "fwd", "bwd")},
        "step_fused_over_torch": round(med["step_fused"] / med["step_torch"], 3),
        "max_rel_diff_fused_vs_composed": agree, "reps": REPS, "rounds": ROUNDS}))


if __name__ == "__main__":
    main()
