"""Timing of the MMOE forward (model/mmoe.py:10-32) at two configurations:

  toy   : the reference's own (model/mmoe.py:35-48): d 4, H 10, E 3, T 3,
          towers [20, 10] -> 1;
  ctr   : d 221 (13 dense + 26 fields x k 8), H 64, E 8, T 2, towers
          [32, 16] -> 1;

both at B 4096, three ways on the same weights, in the same process:

  fused   : forward_fused — ONE rs_mmoe_fwd launch;
  unfused : forward_unfused — rs_dense_fwd for the experts and per gate,
            torch softmax / multiply / sum per task, one rs_mlp_fwd per tower;
  torch   : torch ops only (F.linear, relu, softmax, multiply, sum).

Each variant is replayed from a captured graph (REPS calls per replay; eager
calls if a capture fails), the variants alternate over ROUNDS rounds, times
come from device events and the medians are reported with each variant's min
and max over the rounds.  Prints one JSON line."""
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as TF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import recommender_system_amd as rs  # noqa: E402

REPS = int(os.environ.get("MMOE_REPS", "100"))  # 1-11 ms of device work per timed window
ROUNDS = int(os.environ.get("MMOE_ROUNDS", "9"))

CONFIGS = {
    "toy": dict(d=4, H=10, E=3, T=3, towers=[20, 10], out=1),
    "ctr": dict(d=221, H=64, E=8, T=2, towers=[32, 16], out=1),
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


def time_config(name, cfg, B, dev):
    d, H, E, T, towers, out = (cfg[k] for k in ("d", "H", "E", "T", "towers", "out"))
    m = rs.MMOE(H, E, T, towers, out, device=dev, seed=0, input_dim=d)
    assert m.fused_ok(), name
    gen = torch.Generator(device="cpu").manual_seed(1)
    for tower in m.tower_layer:  # non-zero biases, as a trained model has
        for layer in tower._layers():
            layer.bias.copy_(torch.randn(layer.bias.shape, generator=gen).mul_(0.05))
    m._weights_changed()
    x = torch.randn(B, d, generator=gen).to(dev)
    L = m.mmoe_layer

    def fused():
        return m.forward_fused(x)

    def unfused():
        return m.forward_unfused(x)

    ew = L.expert_matrix.reshape(d, H * E).t().contiguous()
    eb = L.expert_bias.reshape(-1)
    gw = [(g.t().contiguous(), b) for g, b in zip(L.gate_matrix, L.gate_bias)]
    tw = [[(l.kernel.t().contiguous(), l.bias) for l in tower._layers()] for tower in m.tower_layer]

    def torch_ops():
        experts = torch.relu(TF.linear(x, ew, eb)).view(B, H, E)
        ys = []
        for (g, b), tower in zip(gw, tw):
            h = (experts * torch.softmax(TF.linear(x, g, b), dim=-1).unsqueeze(1)).sum(-1)
            for w, bb in tower[:-1]:
                h = torch.relu(TF.linear(h, w, bb))
            ys.append(TF.linear(h, *tower[-1]))
        return ys

    parts = {"fused": fused, "unfused": unfused, "torch": torch_ops}
    outs = {n: torch.stack(list(fn())) for n, fn in parts.items()}
    torch.cuda.synchronize()
    agree = {n: float((outs[n] - outs["unfused"]).abs().max()) for n in parts}

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
    dims = [H] + towers + [out]
    flop = 2 * d * (H + T) * E + T * (2 * H * E + sum(2 * a * b for a, b in zip(dims[:-1], dims[1:])))
    return {
        "workload": f"MMOE d {d} H {H} E {E} T {T} towers {towers} -> {out} B {B}",
        "median_us": {n: round(v, 2) for n, v in med.items()},
        "min_us": {n: round(float(np.min(v)), 2) for n, v in times.items()},
        "max_us": {n: round(float(np.max(v)), 2) for n, v in times.items()},
        "mode": {n: r[1] for n, r in runners.items()},
        "fused_over_unfused": round(med["fused"] / med["unfused"], 3),
        "fused_over_torch": round(med["fused"] / med["torch"], 3),
        "gap_us_min_unfused_minus_max_fused": round(float(np.min(times["unfused"]) - np.max(times["fused"])), 2),
        "kflop_per_sample": round(flop / 1e3, 2),
        "prepared_kb": round(m.prepared().numel() * 4 / 1e3, 1),
        "max_abs_diff_vs_unfused": agree}


def main():
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda")
    B = int(os.environ.get("MMOE_B", "4096"))
    res = {name: time_config(name, cfg, B, dev) for name, cfg in CONFIGS.items()}
    print(json.dumps({"script": "scripts/time_mmoe.py", "reps": REPS, "rounds": ROUNDS, **res}))


if __name__ == "__main__":
    main()
