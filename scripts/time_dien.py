"""Timing of DIEN's interest evolution (model/dien.py:54-80: GRU, attention
scores, AUGRU) at two shapes:

  toy      : the reference's own (model/dien.py:172-213): T 4, D 8 + 4;
  workload : T 50, D 24 + 12 = 36, attention (64, 16), dice, normalised scores;

both at B 4096 with lengths uniform in 1..T, on the same weights, in the same
process:

  fused     : InterestEvolution.forward_fused — ONE rs_dien_evolution_fwd
              launch on gathered keys [B, T, D];
  fused_ids : forward_ids — the same launch from the behaviour ids (the
              model's path: the keys are never written);
  unfused   : forward_unfused — rs_gru_fwd, the composed attention scores
              (rs_dense_fwd per layer + torch glue), rs_augru_fwd;
  torch     : torch ops only for the same math (the baseline: there is no
              earlier DIEN to compare with).

Each variant is replayed from a captured graph (REPS calls per replay; eager
calls if a capture fails), the variants alternate over ROUNDS rounds, times
come from device events and the medians are reported with each variant's min
and max over the rounds.  Prints one JSON line."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import recommender_system_amd as rs  # noqa: E402

REPS = int(os.environ.get("DIEN_REPS", "10"))  # the torch variant is ~20 T launches per call
ROUNDS = int(os.environ.get("DIEN_ROUNDS", "9"))

CONFIGS = {
    "toy": dict(T=4, widths=(8, 4), vocabs=(4, 3), att=(64, 16), act="dice", norm=True),
    "workload": dict(T=50, widths=(24, 12), vocabs=(60000, 800), att=(64, 16), act="dice", norm=True),
}


def runner(fn):
    """fn replayed REPS times from a captured graph ('graph'), or called REPS
    times ('eager') when the capture fails."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    try:
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
        return g.replay, "graph"
    except Exception as ex:  # noqa: BLE001
        torch.cuda.synchronize()
        print(f"capture failed ({type(ex).__name__}: {ex}); eager timing", file=sys.stderr)

        def eager():
            for _ in range(REPS):
                fn()
        return eager, "eager"


def torch_evolution(m, keys, q, L):
    """The same math in torch ops (float32)."""
    w = {k: v for k, v in m.keras_weights().items()}
    B, T, D = keys.shape
    W1, U1, b1 = w["gru1/kernel"], w["gru1/recurrent_kernel"], w["gru1/bias"]
    h = torch.zeros(B, D, device=keys.device)
    xi_all = keys @ W1 + b1[0]
    hs = []
    for t in range(T):
        xi, hr = xi_all[:, t], h @ U1 + b1[1]
        z = torch.sigmoid(xi[:, :D] + hr[:, :D])
        r = torch.sigmoid(xi[:, D:2 * D] + hr[:, D:2 * D])
        h = z * h + (1 - z) * torch.tanh(xi[:, 2 * D:] + r * hr[:, 2 * D:])
        hs.append(h)
    h1 = torch.stack(hs, 1)
    a = m.attention
    p = "attention_sequence_pooling_layer/local_att/"
    qq = q.unsqueeze(1).expand(B, T, D)
    e = torch.cat([qq, h1, qq - h1, qq * h1], -1)
    for i in range(len(a.att_hidden_units)):
        e = e @ w[p + f"dnn/kernel{i}"] + w[p + f"dnn/bias{i}"]
        if a.att_activation == "dice":
            pr = torch.sigmoid((e - w[p + f"dnn/dice{i}/bn/moving_mean"])
                               * torch.rsqrt(w[p + f"dnn/dice{i}/bn/moving_variance"] + 1e-9))
            e = w[p + f"dnn/dice{i}/dice_alpha"] * (1 - pr) * e + pr * e
        else:
            e = torch.relu(e) if a.att_activation == "relu" else torch.sigmoid(e)
    s = (e @ w[p + "kernel"] + w[p + "bias"]).squeeze(-1)
    valid = torch.arange(T, device=keys.device).unsqueeze(0) < L.unsqueeze(1)
    if a.weight_normalization:
        s = torch.softmax(torch.where(valid, s, torch.full_like(s, float(-2 ** 32 + 1))), -1)
    else:
        s = torch.where(valid, s, torch.zeros_like(s))
    W2, U2 = w["gru2/kernel"], w["gru2/recurrent_kernel"]
    xi_all = h1 @ W2
    h = torch.zeros(B, D, device=keys.device)
    hsig = lambda v: torch.clamp(0.2 * v + 0.5, 0, 1)
    for t in range(T):
        xi = xi_all[:, t]
        z = hsig(xi[:, :D] + h @ U2[:, :D]) * s[:, t:t + 1]
        r = hsig(xi[:, D:2 * D] + h @ U2[:, D:2 * D])
        h = z * h + (1 - z) * torch.tanh(xi[:, 2 * D:] + (r * h) @ U2[:, 2 * D:])
    return h


def time_config(name, cfg, B, dev):
    T, widths, vocabs, att = cfg["T"], cfg["widths"], cfg["vocabs"], cfg["att"]
    D = sum(widths)
    m = rs.InterestEvolution(D, att, cfg["act"], cfg["norm"], device=dev, seed=0)
    assert m.fused_ok(T), name
    gen = torch.Generator(device="cpu").manual_seed(1)
    with torch.no_grad():  # a trained model's biases and Dice statistics are not at their initial values
        for k, p in m.keras_weights().items():
            if k.endswith("moving_variance"):
                p.copy_(torch.rand(p.shape, generator=gen) + 0.5)
            elif p.dim() == 1 or k.endswith("gru1/bias"):
                p.copy_(torch.randn(p.shape, generator=gen).mul_(0.1))
    m._weights_changed()
    tabs = [torch.randn(v, k, generator=gen).mul_(0.5).to(dev) for v, k in zip(vocabs, widths)]
    hist = [torch.randint(0, v, (B, T), generator=gen).to(dev) for v in vocabs]
    cand = [torch.randint(0, v, (B,), generator=gen).to(dev) for v in vocabs]
    L = torch.randint(1, T + 1, (B,), generator=gen).to(dev)
    keys = torch.cat([t[h] for t, h in zip(tabs, hist)], -1).contiguous()
    q = torch.cat([t[c] for t, c in zip(tabs, cand)], -1).contiguous()
    out = {n: torch.empty(B, D, device=dev) for n in ("fused", "fused_ids", "unfused")}

    parts = {
        "fused": lambda: m.forward_fused(keys, q, L, out=out["fused"]),
        "fused_ids": lambda: m.forward_ids(hist, cand, tabs, L, out=out["fused_ids"], check_ids=False),
        "unfused": lambda: m.forward_unfused(keys, q, L, out=out["unfused"]),
        "torch": lambda: torch_evolution(m, keys, q, L),
    }
    outs = {n: fn().clone() for n, fn in parts.items()}
    torch.cuda.synchronize()
    agree = {n: float((outs[n] - outs["torch"]).abs().max()) for n in parts}
    assert torch.equal(outs["fused"], outs["fused_ids"])

    runners = {n: runner(fn) for n, fn in parts.items()}
    times = {n: [] for n in parts}
    names = list(parts)
    for r in range(ROUNDS):
        for n in (names if r % 2 == 0 else names[::-1]):
            run = runners[n][0]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run()
            e1.record()
            torch.cuda.synchronize()
            times[n].append(e0.elapsed_time(e1) * 1e3 / REPS)
    med = {n: float(np.median(v)) for n, v in times.items()}
    flop = T * (4 * 2 * D * 3 * D + 2 * (2 * D * att[0]) + 2 * att[0] * att[1] + 2 * att[1]) + 2 * D * att[0]
    return {
        "workload": f"DIEN evolution T {T} D {D} att {list(att)} {cfg['act']} norm {cfg['norm']} B {B}",
        "median_us": {n: round(v, 2) for n, v in med.items()},
        "min_us": {n: round(float(np.min(v)), 2) for n, v in times.items()},
        "max_us": {n: round(float(np.max(v)), 2) for n, v in times.items()},
        "mode": {n: r[1] for n, r in runners.items()},
        "fused_over_unfused": round(med["fused"] / med["unfused"], 3),
        "fused_over_torch": round(med["fused"] / med["torch"], 3),
        "fused_ids_over_torch": round(med["fused_ids"] / med["torch"], 3),
        "gap_us_min_torch_minus_max_fused": round(float(np.min(times["torch"]) - np.max(times["fused"])), 2),
        "kflop_per_sample_fused": round(flop / 1e3, 2),
        "prepared_kb": round(m.prepared().numel() * 4 / 1e3, 1),
        "max_abs_diff_vs_torch": agree}


def main():
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda")
    B = int(os.environ.get("DIEN_B", "4096"))
    res = {name: time_config(name, cfg, B, dev) for name, cfg in CONFIGS.items()}
    print(json.dumps({"script": "scripts/time_dien.py", "reps": REPS, "rounds": ROUNDS, **res}))


if __name__ == "__main__":
    main()
