"""Timing of DeepCrossing at the reference's own configuration
(model/deepCrossing.py:35-45: hidden_units [256, 256], res_layer_num 4; 13
dense + 26 fields x k 8 = 221 inputs) at B 4096, four ways on the same
weights, in the same process:

  fused  : forward_fused — ONE rs_deepcrossing_fwd launch from the ids;
  layers : the composition the library offered before the residual tower:
           rs_embed_gather, rs_dense_fwd per Dense (12 + the sigmoid head),
           torch add / relu per unit;
  units  : rs_embed_gather, one rs_res_tower_fwd per unit, the Dense head
           (forward_unfused);
  torch  : the project's gather, then F.linear / relu / add per layer and
           sigmoid(F.linear) in torch ops.

Each variant is replayed from a captured graph (REPS calls per replay; eager
calls if a capture fails), the variants alternate over ROUNDS rounds, times
come from device events and the medians are reported.  The FLOP count is the
algorithm's (2 * in * out per Dense per sample), the rate is that over the
fused median — a whole-forward rate, not a kernel's share of peak.  Prints one
JSON line."""
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as TF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import recommender_system_amd as rs  # noqa: E402

REPS = int(os.environ.get("DC_REPS", "20"))
ROUNDS = int(os.environ.get("DC_ROUNDS", "9"))


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


def main():
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda")
    B, F, k, nd = int(os.environ.get("DC_B", "4096")), 26, 8, 13
    hidden, n_units = [256, 256], 4
    rng = np.random.default_rng(0)
    vocabs = rng.integers(100, 100000, size=F)
    dense_cols = [{"feat": f"I{i + 1}"} for i in range(nd)]
    sparse_cols = [{"feat": f"C{i + 1}", "feat_onehot_dim": int(v), "embed_dim": k} for i, v in enumerate(vocabs)]
    m = rs.DeepCrossing([dense_cols, sparse_cols], 32, hidden, n_units, embed_dim=k, seed=0)
    assert m.fused_ok()
    gen = torch.Generator(device="cpu").manual_seed(1)
    for unit in m.res_layer:  # non-zero biases, as a trained model has
        for layer in unit._layers():
            layer.bias.copy_(torch.randn(layer.bias.shape, generator=gen).mul_(0.05))
    m._weights_changed()
    ids = torch.as_tensor(np.stack([rng.integers(0, v, B) for v in vocabs], 1).astype(np.int32)).to(dev)
    dense = torch.rand(B, nd, device=dev)
    e = m.embed_layer

    def fused():
        return m.forward_fused((dense, ids), check_ids=False)

    def units():
        return m.forward_unfused((dense, ids), check_ids=False)

    def layers():
        x = e.gather(ids, dense, check_ids=False)
        for unit in m.res_layer:
            x = unit.forward_layers(x)
        return m.output_layer(x)

    tw = [[(l.kernel.t().contiguous(), l.bias) for l in unit._layers()] for unit in m.res_layer]
    th = (m.output_layer.kernel.t().contiguous(), m.output_layer.bias)

    def torch_ops():
        x = e.gather(ids, dense, check_ids=False)
        for unit in tw:
            h = x
            for w, b in unit[:-1]:
                h = torch.relu(TF.linear(h, w, b))
            h = TF.linear(h, *unit[-1])
            x = torch.relu(x + h)
        return torch.sigmoid(TF.linear(x, *th))

    parts = {"fused": fused, "layers": layers, "units": units, "torch": torch_ops}
    outs = {n: fn() for n, fn in parts.items()}
    torch.cuda.synchronize()
    agree = {n: float((outs[n] - outs["layers"]).abs().max()) for n in parts}

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
    dims = [m.d] + hidden + [m.d]
    flop = B * (n_units * sum(2 * a * b for a, b in zip(dims[:-1], dims[1:])) + 2 * m.d)
    print(json.dumps({
        "workload": f"DeepCrossing nd {nd} F {F} k {k} d {m.d} hidden {hidden} x {n_units} B {B}",
        "median_us": {n: round(v, 2) for n, v in med.items()},
        "min_us": {n: round(float(np.min(v)), 2) for n, v in times.items()},
        "max_us": {n: round(float(np.max(v)), 2) for n, v in times.items()},
        "mode": {n: r[1] for n, r in runners.items()},
        "fused_over_layers": round(med["fused"] / med["layers"], 3),
        "fused_over_units": round(med["fused"] / med["units"], 3),
        "fused_over_torch": round(med["fused"] / med["torch"], 3),
        "mflop_per_sample": round(flop / B / 1e6, 4),
        "fused_forward_tflops": round(flop / med["fused"] / 1e6, 2),
        "prepared_mb": round(m.prepared().numel() * 4 / 1e6, 3),
        "max_abs_diff_vs_layers": agree, "reps": REPS, "rounds": ROUNDS}))


if __name__ == "__main__":
    main()
