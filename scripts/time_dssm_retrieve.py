"""Timing of DSSM retrieval (retrieval.topn_inner_product): exact top-N by
inner product of l2-normalised Gaussian rows, E 32, N 50, at

  ml-1m     : U 6040 users x I 3707 items (every user against the catalogue);
  4096x1e6  : U 4096 x I 1 000 000;
  256x1e6   : U 256 x I 1 000 000,

in the same process, on the same matrices:

  kernel : rs_topn_inner_product at auto splits (fused=True);
  torch  : the torch composition (fused=False) — chunked matmul, topk on the
           64-bit (score, ~position) key, topk merge of the chunk results.
           There is no earlier retrieval path, so this is the baseline.

Each variant is replayed from a captured graph (REPS calls per replay; eager
calls if a capture fails), the variants alternate over ROUNDS rounds, times
come from device events and the medians are reported with each variant's min
and max over the rounds.  ``faster`` names a variant only when its slowest
round beats the other's fastest (the ranges do not overlap), else "overlap".
For the kernel: the achieved share of the 157 TF fp32 MFMA peak (2 U I E flop)
and the item bytes it streams (the item matrix once per 64-row user tile).
Prints one JSON line and appends it to profiles/dssm_retrieve_timing.jsonl
(DSSM_OUT names another file)."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import recommender_system_amd as rs  # noqa: E402
from scripts.time_dssm import runner  # noqa: E402

ROUNDS = int(os.environ.get("DSSM_ROUNDS", "7"))
OUT = os.environ.get("DSSM_OUT", os.path.join(ROOT, "profiles", "dssm_retrieve_timing.jsonl"))
PEAK_FLOPS = 157e12  # MI355X fp32 MFMA
E, N = 32, 50
SHAPES = {  # name: (U, I, calls per replay)
    "ml-1m": (6040, 3707, 10),
    "4096x1e6": (4096, 1000000, 2),
    "256x1e6": (256, 1000000, 4),
}
ONLY = [s for s in os.environ.get("DSSM_SHAPES", ",".join(SHAPES)).split(",") if s]


def unit_rows(n, gen, dev):
    x = torch.randn(n, E, generator=gen)
    return (x / x.norm(dim=1, keepdim=True)).to(dev)


def time_shape(name, U, I, reps, gen, dev):
    u, v = unit_rows(U, gen, dev), unit_rows(I, gen, dev)
    parts = {"kernel": lambda: rs.topn_inner_product(u, v, N, fused=True),
             "torch": lambda: rs.topn_inner_product(u, v, N, fused=False)}
    outs = {n: fn() for n, fn in parts.items()}
    torch.cuda.synchronize()
    same_pos = float((outs["kernel"][0] == outs["torch"][0]).to(torch.float32).mean())
    score_diff = float((outs["kernel"][1] - outs["torch"][1]).abs().max())
    del outs
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
    med = {n: float(np.median(t)) for n, t in times.items()}
    lo = {n: float(np.min(t)) for n, t in times.items()}
    hi = {n: float(np.max(t)) for n, t in times.items()}
    faster = "kernel" if hi["kernel"] < lo["torch"] else "torch" if hi["torch"] < lo["kernel"] else "overlap"
    need = rs._lib.lib().rs_topn_inner_product_workspace_size(U, I, N, 0)
    return {
        "workload": f"top-{N} of U {U} x I {I}, E {E}, unit-norm Gaussian rows",
        "median_us": {n: round(t, 1) for n, t in med.items()},
        "min_us": {n: round(t, 1) for n, t in lo.items()},
        "max_us": {n: round(t, 1) for n, t in hi.items()},
        "mode": {n: r[1] for n, r in runners.items()},
        "reps": reps,
        "faster": faster,
        "gap_us_min_torch_minus_max_kernel": round(lo["torch"] - hi["kernel"], 1),
        "torch_over_kernel": round(med["torch"] / med["kernel"], 2),
        "kernel_tflops": round(2.0 * U * I * E / (med["kernel"] * 1e-6) / 1e12, 2),
        "kernel_share_of_157tf": round(2.0 * U * I * E / (med["kernel"] * 1e-6) / PEAK_FLOPS, 4),
        "kernel_item_bytes_streamed": int((U + 63) // 64 * I * E * 4),
        "kernel_item_gb_per_s": round((U + 63) // 64 * I * E * 4 / (med["kernel"] * 1e-6) / 1e9, 1),
        "kernel_splits": int(need // (U * N * 8)) or 1,
        "same_positions_share": round(same_pos, 6),
        "max_abs_score_diff": score_diff}


def main():
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda")
    gen = torch.Generator(device="cpu").manual_seed(1)
    res = {n: time_shape(n, *SHAPES[n], gen, dev) for n in ONLY}
    line = json.dumps({"script": "scripts/time_dssm_retrieve.py", "rounds": ROUNDS, "E": E, "N": N, **res})
    print(line)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
