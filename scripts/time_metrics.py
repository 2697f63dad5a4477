"""Timing of the on-device evaluation metrics (metrics.binary_metrics: log-loss,
accuracy and exact ROC AUC; with group ids also GAUC) on sigmoid(Gaussian)
predictions with Bernoulli(p) labels, at

  1e6      : N 1 000 000;           1e7      : N 10 000 000;
  1e6/g1e5 : N 1e6, 100 000 groups; 1e7/g1e5 : N 1e7, 100 000 groups,

in the same process, on the same tensors:

  kernel : rs_binary_metrics + rs_auc into one result tensor (the two launches
           sequences metrics.binary_metrics makes, without its host read);
  torch  : the torch composition on the same device, written below — fp64
           clamp/log loss, torch.sort, head flags, cumsum, scatter_add per tie
           run (and a second, stable sort by group for GAUC).  There is no
           earlier path, so this is the baseline;
  host   : (ungrouped only) the device-to-host copy followed by
           sklearn.metrics.roc_auc_score, wall clock, HOST_ROUNDS rounds.

kernel and torch are each replayed from a captured graph (REPS calls per
replay; eager calls if a capture fails), alternate over ROUNDS rounds, and are
timed with device events; medians are reported with each variant's min and
max.  ``faster`` names a variant only when its slowest round beats the other's
fastest, else "overlap".  The three AUCs are compared first.  Prints one JSON
line and appends it to profiles/metrics_timing.jsonl (METRICS_OUT names
another file)."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from recommender_system_amd import metrics  # noqa: E402
from scripts.time_dssm import runner  # noqa: E402

ROUNDS = int(os.environ.get("METRICS_ROUNDS", "7"))
HOST_ROUNDS = int(os.environ.get("METRICS_HOST_ROUNDS", "3"))
OUT = os.environ.get("METRICS_OUT", os.path.join(ROOT, "profiles", "metrics_timing.jsonl"))
SHAPES = {  # name: (N, groups, calls per replay)
    "1e6": (1000000, 0, 5),
    "1e7": (10000000, 0, 2),
    "1e6/g1e5": (1000000, 100000, 5),
    "1e7/g1e5": (10000000, 100000, 2),
}
ONLY = [s for s in os.environ.get("METRICS_SHAPES", ",".join(SHAPES)).split(",") if s]
EPS = 1e-7


def torch_metrics(p, y, g, G, out):
    """out[0..4] = loss_sum, n_correct, auc, gauc, P (fp64), no host sync."""
    n = p.numel()
    q = p.double().clamp(EPS, 1.0 - EPS)
    yd = y.double()
    out[0] = -(yd * torch.log(q + EPS) + (1.0 - yd) * torch.log(1.0 - q + EPS)).sum()
    out[1] = ((p > 0.5) == (y == 1)).sum()
    true = torch.ones(1, dtype=torch.bool, device=p.device)
    ss, o1 = torch.sort(p + 0.0)  # (-0.0 + 0.0 == +0.0)
    ys = (y[o1] == 1).long()
    head = torch.cat([true, ss[1:] != ss[:-1]])
    rid = torch.cumsum(head, 0) - 1
    zeros = lambda m: torch.zeros(m, dtype=torch.int64, device=p.device)
    p_r, n_r = zeros(n).scatter_add_(0, rid, ys), zeros(n).scatter_add_(0, rid, 1 - ys)
    below = torch.cumsum(n_r, 0) - n_r
    P = ys.sum()
    out[4] = P
    out[2] = (p_r * (2 * below + n_r)).sum().double() / (2.0 * P.double() * (n - P).double())
    if g is None:
        return
    gs, o2 = torch.sort(g[o1], stable=True)
    ss, ys = ss[o2], ys[o2]
    head = torch.cat([true, (gs[1:] != gs[:-1]) | (ss[1:] != ss[:-1])])
    rid = torch.cumsum(head, 0) - 1
    p_r, n_r = zeros(n).scatter_add_(0, rid, ys), zeros(n).scatter_add_(0, rid, 1 - ys)
    rg = zeros(n).scatter_(0, rid, gs)
    Pg, Qg = zeros(G).scatter_add_(0, gs, ys), zeros(G).scatter_add_(0, gs, 1 - ys)
    below = (torch.cumsum(n_r, 0) - n_r) - (torch.cumsum(Qg, 0) - Qg)[rg]
    u2 = zeros(G).scatter_add_(0, rg, p_r * (2 * below + n_r))
    ok = (Pg > 0) & (Qg > 0)
    size = (Pg + Qg).double()
    term = torch.where(ok, size * u2.double() / (2.0 * Pg.double() * Qg.double()).clamp(min=1.0), 0.0)
    out[3] = term.sum() / (size * ok).sum()


def time_shape(name, N, G, reps, gen, dev):
    z = torch.randn(N, generator=gen)
    p = torch.sigmoid(z).to(dev)
    y = (torch.rand(N, generator=gen) < torch.sigmoid(z)).to(torch.float32).to(dev)
    g = torch.randint(0, G, (N,), generator=gen).to(dev) if G else None
    del z
    res = torch.zeros(24, dtype=torch.int64, device=dev)
    tout = torch.zeros(5, dtype=torch.float64, device=dev)

    def kernel():
        metrics._launch_bm(p, 1, y, 0, res[:8])
        metrics._launch_auc(p, 1, y, g, G, res[8:])

    parts = {"kernel": kernel, "torch": lambda: torch_metrics(p, y, g, G, tout)}
    full = metrics.binary_metrics(p, y, g, G if G else None)
    torch_metrics(p, y, g, G, tout)
    t = tout.tolist()
    check = {"auc_kernel": full["auc"], "auc_torch": t[2], "loss_sum_rel_diff": abs(full["loss_sum"] - t[0]) / t[0],
             "n_correct_equal": full["n_correct"] == int(t[1])}
    if G:
        check.update(gauc_kernel=full["gauc"], gauc_torch=t[3], groups_used=full["groups_used"])
    host = None
    if not G:
        from sklearn.metrics import roc_auc_score
        ts = []
        for _ in range(HOST_ROUNDS):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            auc_host = roc_auc_score(y.cpu().numpy(), p.cpu().numpy())
            ts.append((time.perf_counter() - t0) * 1e6)
        check["auc_host"] = float(auc_host)
        host = {"median_us": round(float(np.median(ts)), 1), "min_us": round(min(ts), 1), "max_us": round(max(ts), 1),
                "rounds": HOST_ROUNDS}
    runners = {n: runner(fn, reps) for n, fn in parts.items()}
    times = {n: [] for n in parts}
    names = list(parts)
    for r in range(ROUNDS):
        for n in (names if r % 2 == 0 else names[::-1]):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            runners[n][0]()
            e1.record()
            torch.cuda.synchronize()
            times[n].append(e0.elapsed_time(e1) * 1e3 / reps)
    med = {n: float(np.median(v)) for n, v in times.items()}
    lo = {n: float(np.min(v)) for n, v in times.items()}
    hi = {n: float(np.max(v)) for n, v in times.items()}
    faster = "kernel" if hi["kernel"] < lo["torch"] else "torch" if hi["torch"] < lo["kernel"] else "overlap"
    lib = metrics._lib.lib()
    out = {"workload": f"N {N}" + (f", {G} groups" if G else "") + ", sigmoid(Gaussian) predictions",
           "median_us": {n: round(v, 1) for n, v in med.items()},
           "min_us": {n: round(v, 1) for n, v in lo.items()},
           "max_us": {n: round(v, 1) for n, v in hi.items()},
           "mode": {n: r[1] for n, r in runners.items()},
           "reps": reps,
           "faster": faster,
           "torch_over_kernel": round(med["torch"] / med["kernel"], 2),
           "kernel_workspace_bytes": int(lib.rs_auc_workspace_size(N, G)),
           "kernel_ns_per_element": round(med["kernel"] * 1e3 / N, 3),
           "check": check}
    if host:
        out["host_roc_auc_score"] = host
        out["host_over_kernel"] = round(host["median_us"] / med["kernel"], 1)
    return out


def main():
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda")
    gen = torch.Generator(device="cpu").manual_seed(1)
    res = {n: time_shape(n, *SHAPES[n], gen, dev) for n in ONLY}
    line = json.dumps({"script": "scripts/time_metrics.py", "rounds": ROUNDS, **res})
    print(line)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
