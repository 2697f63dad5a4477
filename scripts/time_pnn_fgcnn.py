"""Timing of PNN(mode='both', use_fgcnn=True, embed_dim=8), hidden
[256, 128, 64], 26 fields, B 4096 (the reference's own example configuration,
model/pnn.py:56-71), and of its FGCNN front end against the same computation
written with torch ops on the same device, in the same process, with the same
weights:

  hand : rs_embed_fgcnn_conv_fwd (gather + conv stack, one launch) and one
         rs_dense_fwd per FGCNN layer, writing z = [embed | new fields];
  torch: the project's gather, then F.conv2d / tanh / F.max_pool2d / permute to
         Keras Flatten order / F.linear / relu per layer, torch.cat into z.

Each variant is replayed from a captured graph (REPS calls per replay; eager
calls if a capture fails), the variants alternate over ROUNDS rounds, times
come from device events and the medians are reported.  Also: product_inputs,
the full forward, the tower's first layer (rs_dense_fwd 7470 -> 256) and their
shares.  Prints one JSON line."""
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as TF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import recommender_system_amd as rs  # noqa: E402

REPS = int(os.environ.get("FG_REPS", "20"))
ROUNDS = int(os.environ.get("FG_ROUNDS", "9"))


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
    B, F, k = int(os.environ.get("FG_B", "4096")), 26, 8
    rng = np.random.default_rng(0)
    vocabs = rng.integers(100, 100000, size=F)
    dense_cols = [{"feat": f"I{i + 1}"} for i in range(13)]
    sparse_cols = [{"feat": f"C{i + 1}", "feat_onehot_dim": int(v), "embed_dim": k} for i, v in enumerate(vocabs)]
    m = rs.PNN([dense_cols, sparse_cols], "both", [256, 128, 64], 1, "relu", use_fgcnn=True, embed_dim=k, seed=0)
    fg, e = m.fgcnn_layer, m.embed_layer
    ids = torch.as_tensor(np.stack([rng.integers(0, v, B) for v in vocabs], 1).astype(np.int32)).to(dev)
    dense = torch.rand(B, 13, device=dev)
    Fz = m.n_z

    # torch-op weights: conv [Cout, Cin, kw, 1] from Keras [kw, 1, Cin, Cout]; linear [out, in] from Keras (in, out)
    tw = [(w.permute(3, 2, 0, 1).contiguous(), b) for w, b in zip(fg.conv_kernels, fg.conv_biases)]
    tl = [(d.kernel.t().contiguous(), d.bias) for d in fg.dense_layers]
    assert all(kw % 2 == 1 for kw in fg.kernel_width), "symmetric 'same' padding only in the torch composition"

    def torch_conv(emb):
        x, flats = emb.view(B, 1, F, k), []
        for (w, b), kw, pw in zip(tw, fg.kernel_width, fg.pooling_width):
            x = TF.max_pool2d(torch.tanh(TF.conv2d(x, w, b, padding=(kw // 2, 0))), (pw, 1))
            flats.append(x.permute(0, 2, 3, 1).reshape(B, -1))  # Keras Flatten order [H', k, Cout]
        return flats

    def torch_linear(emb, flats):
        return torch.cat([emb.view(B, F * k)] + [torch.relu(TF.linear(f, w, b)) for f, (w, b) in zip(flats, tl)], 1)

    def torch_front():
        emb = e.gather(ids, check_ids=False)
        return torch_linear(emb, torch_conv(emb))

    z = torch.empty(B, Fz * k, device=dev)
    ws = torch.empty(B, fg.ws_size, device=dev)

    def hand_conv():
        fg.conv_ids(ids, e, z, m._err.t, ws=ws)

    def hand_dense():
        fg.recombine(ws, z, col=F * k)

    def hand_front():
        hand_conv()
        hand_dense()

    # the two front ends compute the same z
    hand_front()
    zt = torch_front()
    torch.cuda.synchronize()
    agree = float((z - zt).abs().max() / zt.abs().max())

    emb0 = e.gather(ids, check_ids=False)
    flats0 = torch_conv(emb0)
    x0 = m.product_inputs((dense, ids), check_ids=False)
    first = m.dnn_layer.hidden_layer[0]
    prod_out = torch.empty(B, m.width, device=dev)

    def product_only():
        rs._lib.call("rs_product_fwd", z.data_ptr(), Fz, k, 1, m.outer_product_layer.prepared().data_ptr(),
                     prod_out.data_ptr(), prod_out.stride(0), B, rs._lib.stream())

    parts = {
        "hand_front": hand_front, "torch_front": torch_front,
        "hand_conv": hand_conv, "hand_dense": hand_dense,
        "torch_conv": lambda: torch_conv(emb0), "torch_linear": lambda: torch_linear(emb0, flats0),
        "product": product_only,
        "product_inputs": lambda: m.product_inputs((dense, ids), check_ids=False),
        "tower_first_layer": lambda: first(x0),
        "forward": lambda: m((dense, ids), check_ids=False),
    }
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
    print(json.dumps({
        "workload": f"PNN both use_fgcnn k {k} F {F} -> {Fz} hidden [256,128,64] B {B}",
        "median_us": {n: round(v, 2) for n, v in med.items()},
        "min_us": {n: round(float(np.min(v)), 2) for n, v in times.items()},
        "max_us": {n: round(float(np.max(v)), 2) for n, v in times.items()},
        "mode": {n: r[1] for n, r in runners.items()},
        "hand_over_torch_front": round(med["hand_front"] / med["torch_front"], 3),
        "share_of_forward": {n: round(med[n] / med["forward"], 3)
                             for n in ("hand_front", "product", "tower_first_layer")},
        "front_ends_max_rel_diff": agree, "reps": REPS, "rounds": ROUNDS}))


if __name__ == "__main__":
    main()
