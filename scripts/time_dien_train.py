"""Timing of DIEN.train_step (protocol of scripts/time_dien.py) at two shapes:

  toy      : the reference's own (model/dien.py:172-213): T 4, D 8 + 4;
  workload : T 50, D 24 + 12 = 36, attention (64, 16), dice, normalised scores;

both at B 4096 with lengths uniform in 1..T, tower (256, 128, 64) relu, dropout
off, in the same process:

  step      : DIEN.train_step, use_negsampling off;
  step_neg  : DIEN.train_step, use_negsampling on (alpha 1);
  torch     : the math of ``step`` as torch ops in float32 with torch.autograd
              and a manual SGD on the same weights (the baseline: there is no
              earlier DIEN training to compare with).

Each variant is replayed from a captured graph (REPS calls per replay; eager
calls if a capture fails — the line says which), the variants alternate over
ROUNDS rounds, times come from device events and the medians are reported with
each variant's min and max over the rounds.  Before the timing, one step of
``step`` and of ``torch`` from the same weights: the largest scaled difference
between the two sets of weights is recorded (not gated).  Appends one JSON line
to profiles/dien_train_timing.jsonl.  DIEN_PROFILE=1: a few eager steps of
``step_neg`` at the workload shape and nothing else (for a kernel trace)."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import recommender_system_amd as rs  # noqa: E402

REPS = int(os.environ.get("DIEN_REPS", "3"))
ROUNDS = int(os.environ.get("DIEN_ROUNDS", "9"))
LR = 0.01
ATT = "attention_sequence_pooling_layer/local_att/"

CONFIGS = {
    "toy": dict(T=4, widths=(8, 4), vocabs=(4, 3)),
    "workload": dict(T=50, widths=(24, 12), vocabs=(60000, 800)),
}


def runner(fn):
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


def build(cfg, neg, dev):
    S, V = rs.SparseFeat, rs.VarLenSparseFeat
    T, (wi, wc), (vi, vc) = cfg["T"], cfg["widths"], cfg["vocabs"]
    cols = [S("user", 1000, embedding_dim=8), S("item", vi, embedding_dim=wi), S("cate", vc, embedding_dim=wc),
            rs.DenseFeat("price", 1)]
    for p in ("", "neg_") if neg else ("",):
        cols += [V(S(p + "hist_item", vi, embedding_dim=wi, embedding_name="item"), maxlen=T, length_name="seq_length"),
                 V(S(p + "hist_cate", vc, embedding_dim=wc, embedding_name="cate"), maxlen=T, length_name="seq_length")]
    return rs.DIEN(cols, ["item", "cate"], use_negsampling=neg, att_hidden_units=(64, 16), att_activation="dice",
                   att_weight_normalization=True, l2_reg_embedding=0, device=dev, seed=3)


def data(cfg, B, dev):
    gen = torch.Generator(device="cpu").manual_seed(1)
    T, (vi, vc) = cfg["T"], cfg["vocabs"]
    ri = lambda hi, *s: torch.randint(0, hi, s, generator=gen).to(dev)
    x = {"user": ri(1000, B), "item": ri(vi, B), "cate": ri(vc, B), "price": torch.randn(B, generator=gen).to(dev),
         "hist_item": ri(vi, B, T), "hist_cate": ri(vc, B, T), "neg_hist_item": ri(vi, B, T),
         "neg_hist_cate": ri(vc, B, T), "seq_length": (ri(T, B) + 1)}
    return x, (torch.rand(B, generator=gen) < 0.3).float().to(dev)


def randomise(m):
    """Tables N(0, 0.5) and non-zero biases / statistics: a trained model's are not at their initial values."""
    gen = torch.Generator(device="cpu").manual_seed(2)
    with torch.no_grad():
        for k, p in m.keras_weights().items():
            if k.endswith("moving_variance"):
                p.copy_(torch.rand(p.shape, generator=gen) + 0.5)
            elif k.endswith("embeddings"):
                p.copy_(torch.randn(p.shape, generator=gen).mul_(0.5))
            elif p.dim() == 1 or k.endswith("gru1/bias"):
                p.copy_(torch.randn(p.shape, generator=gen).mul_(0.1))
    m._weights_changed()


def torch_step(w, x, y, T, D, n_dnn):
    """One SGD step of the model without the auxiliary loss, torch ops and autograd (float32)."""
    train = [k for k in w if not k.endswith(("moving_mean", "moving_variance"))]
    for k in train:
        w[k].requires_grad_(True)
    emb = lambda n, ids: w[n][ids]
    ti, tc = "sparse_seq_emb_hist_item/embeddings", "sparse_seq_emb_hist_cate/embeddings"
    keys = torch.cat([emb(ti, x["hist_item"]), emb(tc, x["hist_cate"])], -1)
    q = torch.cat([emb(ti, x["item"]), emb(tc, x["cate"])], -1)
    B = q.shape[0]
    W1, U1, b1 = w["gru1/kernel"], w["gru1/recurrent_kernel"], w["gru1/bias"]
    h, xi_all, hs = torch.zeros(B, D, device=q.device), keys @ W1 + b1[0], []
    for t in range(T):
        xi, hr = xi_all[:, t], h @ U1 + b1[1]
        z = torch.sigmoid(xi[:, :D] + hr[:, :D])
        r = torch.sigmoid(xi[:, D:2 * D] + hr[:, D:2 * D])
        h = z * h + (1 - z) * torch.tanh(xi[:, 2 * D:] + r * hr[:, 2 * D:])
        hs.append(h)
    h1 = torch.stack(hs, 1)
    qq = q.unsqueeze(1).expand(B, T, D)
    e = torch.cat([qq, h1, qq - h1, qq * h1], -1).reshape(B * T, 4 * D)
    moved = {}
    for i in range(2):
        e = e @ w[ATT + f"dnn/kernel{i}"] + w[ATT + f"dnn/bias{i}"]
        mean, var = e.mean(0), e.var(0, unbiased=False)
        for s, v in (("moving_mean", mean), ("moving_variance", var)):
            moved[ATT + f"dnn/dice{i}/bn/{s}"] = v.detach()
        pr = torch.sigmoid((e - mean) * torch.rsqrt(var + 1e-9))
        e = w[ATT + f"dnn/dice{i}/dice_alpha"] * (1 - pr) * e + pr * e
    s = (e @ w[ATT + "kernel"] + w[ATT + "bias"]).reshape(B, T)
    valid = torch.arange(T, device=q.device).unsqueeze(0) < x["seq_length"].unsqueeze(1)
    s = torch.softmax(torch.where(valid, s, torch.full_like(s, float(-2 ** 32 + 1))), -1)
    W2, U2 = w["gru2/kernel"], w["gru2/recurrent_kernel"]
    xi_all, h = h1 @ W2, torch.zeros(B, D, device=q.device)
    hsig = lambda v: torch.clamp(0.2 * v + 0.5, 0, 1)
    for t in range(T):
        xi = xi_all[:, t]
        z = hsig(xi[:, :D] + h @ U2[:, :D]) * s[:, t:t + 1]
        r = hsig(xi[:, D:2 * D] + h @ U2[:, D:2 * D])
        h = z * h + (1 - z) * torch.tanh(xi[:, 2 * D:] + (r * h) @ U2[:, 2 * D:])
    e = torch.cat([emb("sparse_emb_user/embeddings", x["user"]), emb(ti, x["item"]), emb(tc, x["cate"]), h,
                   x["price"].reshape(B, 1)], -1)
    for i in range(n_dnn):
        e = torch.relu(e @ w[f"dnn/kernel{i}"] + w[f"dnn/bias{i}"])
    logit = (e @ w["dense/kernel"] + w["prediction_layer/global_bias"]).reshape(B)
    loss = torch.nn.functional.binary_cross_entropy_with_logits(logit, y)
    grads = torch.autograd.grad(loss, [w[k] for k in train])
    with torch.no_grad():
        for k, g in zip(train, grads):
            w[k].sub_(LR * g)
        for k, v in moved.items():
            w[k].mul_(0.99).add_(0.01 * v)
    for k in train:
        w[k].requires_grad_(False)


def time_config(name, cfg, B, dev):
    T, D = cfg["T"], sum(cfg["widths"])
    x, y = data(cfg, B, dev)
    m, mn = build(cfg, False, dev), build(cfg, True, dev)
    randomise(m), randomise(mn)
    xs = {k: v for k, v in x.items() if not k.startswith("neg_")}
    w = {k: v.detach().clone() for k, v in m.keras_weights().items()}
    # one step of each from the same weights
    m.train_step(xs, y, lr=LR, dropout=False, check_ids=False)
    torch_step(w, xs, y, T, D, 3)
    torch.cuda.synchronize()

    def scaled(a, b):
        rms = float(b.double().pow(2).mean().sqrt())
        return float(((a.double() - b.double()).abs() / b.double().abs().clamp_min(max(rms, 1e-30))).max())
    diffs = {k: scaled(v, w[k]) for k, v in m.keras_weights().items()}
    worst = max(diffs, key=diffs.get)

    parts = {
        "step": lambda: m.train_step(xs, y, lr=LR, dropout=False, check_ids=False),
        "step_neg": lambda: mn.train_step(x, y, lr=LR, dropout=False, check_ids=False),
        "torch": lambda: torch_step(w, xs, y, T, D, 3),
    }
    runners = {n: runner(fn) for n, fn in parts.items()}
    times = {n: [] for n in parts}
    names = list(parts)
    for r in range(ROUNDS):
        for n in (names if r % 2 == 0 else names[::-1]):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            runners[n][0]()
            e1.record()
            torch.cuda.synchronize()
            times[n].append(e0.elapsed_time(e1) * 1e3 / REPS)
    med = {n: float(np.median(v)) for n, v in times.items()}
    lib = rs._lib.lib()
    return {
        "workload": f"DIEN train_step T {T} D {D} att [64, 16] dice norm True tower [256, 128, 64] B {B}",
        "median_us": {n: round(v, 1) for n, v in med.items()},
        "min_us": {n: round(float(np.min(v)), 1) for n, v in times.items()},
        "max_us": {n: round(float(np.max(v)), 1) for n, v in times.items()},
        "mode": {n: r[1] for n, r in runners.items()},
        "step_over_torch": round(med["step"] / med["torch"], 3),
        "gap_us_min_torch_minus_max_step": round(float(np.min(times["torch"]) - np.max(times["step"])), 1),
        "saved_mb": {"gru": round(lib.rs_gru_saved_size(T, D, D, B) * 4 / 1e6, 2),
                     "augru": round(lib.rs_augru_saved_size(T, D, D, B) * 4 / 1e6, 2)},
        "max_scaled_weight_diff_after_one_step": {"value": diffs[worst], "weight": worst}}


def main():
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda")
    B = int(os.environ.get("DIEN_B", "4096"))
    if os.environ.get("DIEN_PROFILE"):
        cfg = CONFIGS["workload"]
        x, y = data(cfg, B, dev)
        mn = build(cfg, True, dev)
        randomise(mn)
        for _ in range(5):
            mn.train_step(x, y, lr=LR, dropout=False, check_ids=False)
        torch.cuda.synchronize()
        return
    res = {name: time_config(name, cfg, B, dev) for name, cfg in CONFIGS.items()}
    line = json.dumps({"script": "scripts/time_dien_train.py", "reps": REPS, "rounds": ROUNDS, **res})
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "dien_train_timing.jsonl"), "a") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
