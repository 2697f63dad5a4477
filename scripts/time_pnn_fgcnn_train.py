"""Timing of one training step of PNN(mode='both', use_fgcnn=True,
train_fgcnn=True, embed_dim=8), hidden [256, 128, 64], 26 -> 83 fields, B 4096
(the reference's own example configuration, model/pnn.py:56-71), of its parts,
and of the two new backward blocks against torch autograd on the torch-op
composition of the same graph, in the same process, with the same weights:

  front end : FGCNNLayer.backward (relu masks, rs_gemm / rs_col_sum of the
              recombination Dense layers, ONE rs_fgcnn_conv_bwd launch) against
              autograd through F.conv2d / tanh / F.max_pool2d / F.linear / relu;
  products  : rs_product_bwd + rs_product_w_grad against autograd through the
              gathered-pair form of the inner and outer products on z.

Each variant is replayed from a captured graph (REPS calls per replay; eager
calls if a capture fails), the variants alternate over ROUNDS rounds, times
come from device events and the medians are reported with the rounds' spread.
Prints one JSON line."""
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as TF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import recommender_system_amd as rs  # noqa: E402
from recommender_system_amd import _train_ops as T  # noqa: E402
from recommender_system_amd._lib import call, ptr  # noqa: E402

REPS = int(os.environ.get("FG_REPS", "5"))
ROUNDS = int(os.environ.get("FG_ROUNDS", "9"))


def runner(fn):
    """fn replayed REPS times from a captured graph ('graph'), or called REPS
    times ('eager') when the capture fails."""
    for _ in range(2):
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


def rel_diff(a, b):
    return float((a - b).abs().max() / b.abs().max())


def main():
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda")
    B, F, k = int(os.environ.get("FG_B", "4096")), 26, 8
    rng = np.random.default_rng(0)
    vocabs = rng.integers(100, 100000, size=F)
    dense_cols = [{"feat": f"I{i + 1}"} for i in range(13)]
    sparse_cols = [{"feat": f"C{i + 1}", "feat_onehot_dim": int(v), "embed_dim": k} for i, v in enumerate(vocabs)]
    m = rs.PNN([dense_cols, sparse_cols], "both", [256, 128, 64], 1, "relu", use_fgcnn=True, train_fgcnn=True,
               embed_dim=k, seed=0)
    with torch.no_grad():  # logits inside the loss's clip range, so the step carries a gradient
        m.dnn_layer.output_layer.bias.fill_(0.5)
        m.dnn_layer.output_layer.kernel.mul_(0.1)
    fg, op, dnn = m.fgcnn_layer, m.outer_product_layer, m.dnn_layer
    ids = torch.as_tensor(np.stack([rng.integers(0, v, B) for v in vocabs], 1).astype(np.int32)).to(dev)
    dense = torch.rand(B, 13, device=dev)
    labels = torch.as_tensor(rng.integers(0, 2, B).astype(np.float32)).to(dev)
    Fz, stream = m.n_z, rs._lib.stream  # (asked at every call: a capture runs on its own stream)
    emp = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)

    # one forward's saved tensors and a fixed upstream gradient for the parts
    keep = {}
    x = m.product_inputs((dense, ids), check_ids=False, keep=keep)
    z, ws = keep["z"], keep["ws"]
    delta = torch.randn(B, m.width, device=dev) / B
    dz, dW, de = emp(B, Fz * k), emp(*op.W.shape), emp(B, F * k)
    dnew = torch.randn(B, (Fz - F) * k, device=dev) / B

    def product_bwd():
        call("rs_product_bwd", ptr(z), z.stride(0), ptr(delta), m.width, Fz, k, 1, ptr(op.W), B, ptr(dz), dz.stride(0),
             stream())

    def w_grad():
        call("rs_product_w_grad", ptr(z), z.stride(0), ptr(delta), m.width, Fz, k, 1, B, ptr(dW), stream())

    def front_bwd():
        de.zero_()
        return fg.backward(z, ws, z[:, F * k:], dnew, de)

    dws = emp(B, fg.ws_size)
    dcw, dcb = [torch.empty_like(w) for w in fg.conv_kernels], [torch.empty_like(b) for b in fg.conv_biases]
    cws = torch.empty(fg.bwd_workspace_size(B), dtype=torch.uint8, device=dev)
    gw = T.gemm_ws(fg, T.gemm_need([(*d.kernel.shape, B) for d in fg.dense_layers]))

    def recombination():
        off, col, st = 0, 0, stream()
        for (H, kk, cout), d in zip(fg.pooled_shapes, fg.dense_layers):
            n, u = H * kk * cout, d.units
            dpre = dnew[:, col:col + u] * (z[:, F * k + col:F * k + col + u] > 0)
            T.dense_backward(d.kernel, ws[:, off:off + n], dpre, gw, emp, st, d_in=False)
            call("rs_gemm", 0, 1, B, n, u, 1.0, ptr(dpre), u, ptr(d.kernel), u, 0.0, dws.data_ptr() + 4 * off,
                 fg.ws_size, None, 0, *gw, st)
            off, col = off + n, col + u

    def conv_bwd():
        call("rs_fgcnn_conv_bwd", ptr(z), z.stride(0), ptr(ws), ws.stride(0), ptr(dws), dws.stride(0), F, k,
             *fg._cfg(), rs._lib.ptrs(fg.conv_kernels), ptr(de), de.stride(0), rs._lib.ptrs(dcw), rs._lib.ptrs(dcb),
             ptr(cws), cws.numel(), B, stream())

    layers = list(dnn.hidden_layer) + [dnn.output_layer]
    tgw = T.gemm_ws(m, T.gemm_need([(*L.kernel.shape, B) for L in layers]))
    g = emp(B)

    def tower():
        st = stream()
        acts, _ = T._dnn_train_forward(m, dnn, x, 0.0, st)
        pre = dnn.output_layer(acts[-1])
        call("rs_bce_prob_grad", ptr(pre), pre.stride(0), ptr(labels), B, ptr(g), None, st)
        T._dnn_backward(layers, acts, g.view(B, 1), tgw, emp, st)

    # ---- torch-op compositions with autograd, same weights
    tw = [(w.permute(3, 2, 0, 1).contiguous().requires_grad_(), b.clone().requires_grad_())
          for w, b in zip(fg.conv_kernels, fg.conv_biases)]
    tl = [(d.kernel.t().contiguous().requires_grad_(), d.bias.clone().requires_grad_()) for d in fg.dense_layers]
    assert all(kw % 2 == 1 for kw in fg.kernel_width), "symmetric 'same' padding only in the torch composition"
    emb_t = z[:, :F * k].clone().requires_grad_()
    front_leaves = [emb_t] + [t for pair in tw + tl for t in pair]

    def torch_front_fwd():
        xx, outs = emb_t.view(B, 1, F, k), []
        for (w, b), (lw, lb), kw, pw in zip(tw, tl, fg.kernel_width, fg.pooling_width):
            xx = TF.max_pool2d(torch.tanh(TF.conv2d(xx, w, b, padding=(kw // 2, 0))), (pw, 1))
            outs.append(torch.relu(TF.linear(xx.permute(0, 2, 3, 1).reshape(B, -1), lw, lb)))
        return torch.cat(outs, 1)

    def torch_front_bwd():  # autograd needs its own forward: timed with it, and the forward alone beside it
        return torch.autograd.grad(torch_front_fwd(), front_leaves, dnew)

    iu = torch.triu_indices(Fz, Fz, 1, device=dev)
    z_t = z.clone().view(B, Fz, k).requires_grad_()
    W_t = op.W.clone().requires_grad_()

    def torch_product_fwd():
        p, q = z_t[:, iu[0]], z_t[:, iu[1]]
        inner = (p * q).sum(-1)
        # o_p = q_p^T (W_p p_p): one batched matmul over the pairs, W[a,p,j] as [p, j, a]
        outer = (torch.bmm(p.transpose(0, 1), W_t.permute(1, 2, 0)).transpose(0, 1) * q).sum(-1)
        return torch.cat([z_t.view(B, -1), inner, outer], 1)

    def torch_product_bwd():
        return torch.autograd.grad(torch_product_fwd(), [z_t, W_t], delta)

    def no_grad(fn):
        def run():
            with torch.no_grad():
                return fn()
        return run

    # the two forms agree
    grads_h = front_bwd()
    grads_t = torch_front_bwd()
    pdz, pdW = torch_product_bwd()
    product_bwd()
    w_grad()
    torch.cuda.synchronize()
    agree = {
        "front_de": rel_diff(de, grads_t[0]),
        "front_conv0_kernel": rel_diff(grads_h["conv_0/kernel"], grads_t[1].permute(2, 3, 1, 0)),
        "front_dense1_kernel": rel_diff(grads_h["dense_1/kernel"], grads_t[7].t()),
        "product_dz": rel_diff(dz, pdz.reshape(B, -1)),
        "product_dW": rel_diff(dW, pdW),
    }

    parts = {
        "train_step": lambda: m.train_step((dense, ids), labels, check_ids=False),
        "gradients": lambda: m._gradients((dense, ids), labels, False, False, "gradients"),
        "forward": lambda: m((dense, ids), check_ids=False),
        "front_bwd": front_bwd, "torch_front_bwd": torch_front_bwd, "torch_front_fwd": no_grad(torch_front_fwd),
        "recombination_gemms": recombination, "conv_bwd": conv_bwd,
        "product_bwd": product_bwd, "w_grad": w_grad, "torch_product_bwd": torch_product_bwd,
        "torch_product_fwd": no_grad(torch_product_fwd),
        "tower_fwd_bwd": tower,
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
        "workload": f"PNN both use_fgcnn train k {k} F {F} -> {Fz} hidden [256,128,64] B {B}",
        "median_us": {n: round(v, 2) for n, v in med.items()},
        "min_us": {n: round(float(np.min(v)), 2) for n, v in times.items()},
        "max_us": {n: round(float(np.max(v)), 2) for n, v in times.items()},
        "mode": {n: r[1] for n, r in runners.items()},
        # against autograd's forward + backward, and against that minus the forward alone
        "hand_over_torch_front_bwd": round(med["front_bwd"] / med["torch_front_bwd"], 3),
        "hand_over_torch_front_bwd_less_fwd":
            round(med["front_bwd"] / max(med["torch_front_bwd"] - med["torch_front_fwd"], 1e-9), 3),
        "hand_over_torch_product_bwd": round((med["product_bwd"] + med["w_grad"]) / med["torch_product_bwd"], 3),
        "hand_over_torch_product_bwd_less_fwd":
            round((med["product_bwd"] + med["w_grad"]) / max(med["torch_product_bwd"] - med["torch_product_fwd"], 1e-9),
                  3),
        "share_of_train_step": {n: round(med[n] / med["train_step"], 3)
                                for n in ("forward", "front_bwd", "conv_bwd", "recombination_gemms", "product_bwd",
                                          "w_grad", "tower_fwd_bwd")},
        "max_rel_diff": agree, "reps": REPS, "rounds": ROUNDS}))


if __name__ == "__main__":
    main()
