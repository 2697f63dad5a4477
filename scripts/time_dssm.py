"""Timing of the DSSM forward (model/dssm.py:17-90) at the reference's demo
shape — user tower 5 x 16 + 2 sequences x 32 at T 50 -> 128 -> 64 -> 32, item
tower 2 x 32 -> 64 -> 32, in-batch softmax at temperature 0.05 — with
ml-1m-sized vocabularies, at B 256 (the reference's batch) and B 4096, lengths
uniform in 1..50, on the same weights, in the same process:

  fused   : DSSM.forward — one rs_dssm_tower_fwd launch per tower (ids to the
            normalised embedding) and one rs_inbatch_softmax_fwd;
  unfused : DSSM.forward_unfused — rs_concat_pieces + rs_seq_pool_fwd into a
            [B, width] buffer, rs_mlp_fwd, rs_l2_normalize_fwd per tower, then
            the same loss launch;
  torch   : torch ops only for the same math (the baseline: there is no
            earlier DSSM to compare with);
  user_tower : the fused user tower alone, for its achieved bytes/s against
            the algorithmic bytes (ids and lengths read, the valid sequence
            rows only, the profile rows, the output) and the 8 TB/s peak.

Each variant is replayed from a captured graph (REPS calls per replay; eager
calls if a capture fails), the variants alternate over ROUNDS rounds, times
come from device events and the medians are reported with each variant's min
and max over the rounds.  Prints one JSON line and appends it to
profiles/dssm_timing.jsonl (DSSM_OUT names another file)."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import recommender_system_amd as rs  # noqa: E402

REPS = int(os.environ.get("DSSM_REPS", "20"))
ROUNDS = int(os.environ.get("DSSM_ROUNDS", "9"))
BATCHES = [int(b) for b in os.environ.get("DSSM_B", "256,4096").split(",")]
OUT = os.environ.get("DSSM_OUT", os.path.join(ROOT, "profiles", "dssm_timing.jsonl"))
PEAK_BYTES_PER_S = 8e12  # MI355X HBM3E

T = 50
VOCAB = dict(user_id=6041, gender=3, age=8, occupation=22, zip=3440, movie_id=3707, genres=19)  # ml-1m, ids from 1
PROFILE = ("user_id", "gender", "age", "occupation", "zip")


def runner(fn, reps=None):
    """fn replayed reps (default REPS) times from a captured graph ('graph'),
    or called reps times ('eager') when the capture fails."""
    reps = REPS if reps is None else int(reps)
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
                for _ in range(reps):
                    fn()
        torch.cuda.synchronize()
        return g.replay, "graph"
    except Exception as ex:  # noqa: BLE001
        torch.cuda.synchronize()
        print(f"capture failed ({type(ex).__name__}: {ex}); eager timing", file=sys.stderr)

        def eager():
            for _ in range(reps):
                fn()
        return eager, "eager"


def build_model(dev):
    S, V = rs.SparseFeat, rs.VarLenSparseFeat
    user = [S(n, VOCAB[n], 16) for n in PROFILE] + [
        V(S("hist_movie_id", VOCAB["movie_id"], 32, embedding_name="movie_id"), T, "mean", "hist_len"),
        V(S("hist_genres", VOCAB["genres"], 32, embedding_name="genres"), T, "mean", "hist_len")]
    item = [S("movie_id", VOCAB["movie_id"], 32), S("genres", VOCAB["genres"], 32)]
    gen = torch.Generator(device="cpu").manual_seed(1)
    counts = torch.randint(1, 500, (VOCAB["movie_id"],), generator=gen).tolist()
    m = rs.DSSM(user, item, user_dnn_hidden_units=(128, 64, 32), item_dnn_hidden_units=(64, 32), loss_type="softmax",
                temperature=0.05, sampler_config=rs.NegativeSampler("inbatch", 255, "movie_id", item_count=counts),
                device=dev, seed=0)
    with torch.no_grad():  # a trained model's tables and biases are not at their initial values
        for k, p in m.keras_weights().items():
            if k.endswith("embeddings"):
                p.copy_(torch.randn(p.shape, generator=gen).mul_(0.5))
            elif p.dim() == 1:
                p.copy_(torch.randn(p.shape, generator=gen).mul_(0.1))
    m._weights_changed()
    return m, gen


def make_inputs(B, gen, dev):
    L = torch.randint(1, T + 1, (B,), generator=gen)
    valid = torch.arange(T).unsqueeze(0) < L.unsqueeze(1)
    x = {n: torch.randint(1, VOCAB[n], (B,), generator=gen) for n in PROFILE + ("movie_id", "genres")}
    x["hist_movie_id"] = torch.randint(1, VOCAB["movie_id"], (B, T), generator=gen) * valid  # padded with 0
    x["hist_genres"] = torch.randint(1, VOCAB["genres"], (B, T), generator=gen) * valid
    x["hist_len"] = L
    return {k: v.to(dev) for k, v in x.items()}, int(L.sum())


def torch_tower(m, tw, x):
    parts = [m.tables[c.embedding_name][x[c.name]] for c in tw.sparse_cols]
    for c in tw.varlen_cols:
        e = m.tables[c.embedding_name][x[c.name]]
        L = x[c.length_name]
        mask = (torch.arange(c.maxlen, device=e.device).unsqueeze(0) < L.unsqueeze(1)).to(torch.float32).unsqueeze(-1)
        parts.append((e * mask).sum(1) / (L.to(torch.float32).unsqueeze(1) + 1e-8))
    e = torch.cat(parts, -1)
    n = len(tw.dnn.layers)
    for i, l in enumerate(tw.dnn.layers):
        e = e @ l.kernel + l.bias
        if i < n - 1:
            e = torch.relu(e)
    return e * torch.rsqrt(torch.clamp((e * e).sum(-1, keepdim=True), min=1e-12))


def torch_dssm(m, x):
    """The same math in torch ops (float32)."""
    u, v = torch_tower(m, m.user_tower, x), torch_tower(m, m.item_tower, x)
    z = (u / m.temperature) @ v.t() - m.softmax.logq[x["movie_id"]].unsqueeze(0)
    return (torch.logsumexp(z, dim=1) - torch.diagonal(z)).unsqueeze(1)


def time_batch(m, gen, B, dev):
    x, n_valid = make_inputs(B, gen, dev)
    parts = {
        "fused": lambda: m.forward(x, check_ids=False),
        "unfused": lambda: m.forward_unfused(x, check_ids=False),
        "torch": lambda: torch_dssm(m, x),
        "user_tower": lambda: m.user_embedding(x, check_ids=False),
    }
    outs = {n: fn().clone() for n, fn in parts.items()}
    torch.cuda.synchronize()
    assert torch.equal(outs["fused"], outs["unfused"])
    agree = {n: float((outs[n] - outs["torch"]).abs().max()) for n in ("fused", "unfused")}

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
    lo = {n: float(np.min(v)) for n, v in times.items()}
    hi = {n: float(np.max(v)) for n, v in times.items()}
    # the user tower's algorithmic bytes: ids (int64) and the length, the profile rows, the valid sequence rows, the output
    isz = x["hist_movie_id"].element_size()
    tower_bytes = B * (5 * isz + x["hist_len"].element_size() + 5 * 16 * 4 + 32 * 4) + n_valid * 2 * (isz + 32 * 4)
    rate = tower_bytes / (med["user_tower"] * 1e-6)
    return {
        "workload": f"DSSM demo towers, ml-1m vocabularies, T {T}, in-batch softmax t {m.temperature}, B {B}",
        "median_us": {n: round(v, 2) for n, v in med.items()},
        "min_us": {n: round(v, 2) for n, v in lo.items()},
        "max_us": {n: round(v, 2) for n, v in hi.items()},
        "mode": {n: r[1] for n, r in runners.items()},
        "fused_over_unfused": round(med["fused"] / med["unfused"], 3),
        "unfused_over_torch": round(med["unfused"] / med["torch"], 3),
        "gap_us_min_unfused_minus_max_fused": round(lo["unfused"] - hi["fused"], 2),
        "gap_us_min_torch_minus_max_unfused": round(lo["torch"] - hi["unfused"], 2),
        "fused_faster_than_unfused": hi["fused"] < lo["unfused"],
        "unfused_faster_than_torch": hi["unfused"] < lo["torch"],
        "user_tower_bytes_per_sample": round(tower_bytes / B, 1),
        "user_tower_gb_per_s": round(rate / 1e9, 1),
        "user_tower_share_of_8tb_per_s": round(rate / PEAK_BYTES_PER_S, 4),
        "mean_length": round(n_valid / B, 2),
        "max_abs_diff_vs_torch": agree}


def main():
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda")
    m, gen = build_model(dev)
    res = {f"B{B}": time_batch(m, gen, B, dev) for B in BATCHES}
    line = json.dumps({"script": "scripts/time_dssm.py", "reps": REPS, "rounds": ROUNDS, **res})
    print(line)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
