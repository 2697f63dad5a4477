"""Timing of DSSM.train_step (model/dssm.py:149-152: Adam on the batch mean of
the in-batch softmax losses) at the shape scripts/time_dssm.py times the
forward at — the reference's demo towers, ml-1m-sized vocabularies, T 50,
temperature 0.05 — at B 256 (the reference's batch) and B 4096, on the same
weights, in the same process:

  train_step : DSSM.train_step(check_ids=False) — the tower inputs, the towers
               in training mode, rs_inbatch_softmax_train_fwd / _bwd,
               rs_l2_normalize_bwd, the towers backward,
               rs_embedding_grad_accum per id source, rs_adam_update_multi
               over every parameter (the whole tables, as Keras);
  torch      : the same step in torch ops: autograd on the float32 restatement
               (the tables' l2 as a loss term, so their gradients are dense
               too) and torch.optim.Adam(eps=1e-7, capturable=True).

Each variant is replayed from a captured graph (REPS steps per replay; eager
calls if a capture fails), the variants alternate over ROUNDS rounds, times
come from device events and the medians are reported with each variant's min
and max over the rounds.  Prints one JSON line and appends it to
profiles/dssm_train_timing.jsonl (DSSM_OUT names another file).
DSSM_TRAIN_PROFILE=1 runs five eager train_steps at the first batch size and
nothing else: the body of a rocprofv3 --kernel-trace --stats run."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import recommender_system_amd as rs  # noqa: E402,F401
from time_dssm import T, build_model, make_inputs, runner, torch_tower  # noqa: E402

REPS = int(os.environ.get("DSSM_REPS", "10"))
ROUNDS = int(os.environ.get("DSSM_ROUNDS", "9"))
BATCHES = [int(b) for b in os.environ.get("DSSM_B", "256,4096").split(",")]
OUT = os.environ.get("DSSM_OUT", os.path.join(ROOT, "profiles", "dssm_train_timing.jsonl"))


class TorchStep:
    """The same step on copies of the model's weights: autograd + torch.optim.Adam."""

    def __init__(self, m):
        self.m = m
        self.w = {k: p.detach().clone().requires_grad_(True) for k, p in m.keras_weights().items()}
        self.tables = {en: self.w[f"{kn}/embeddings"] for en, kn in m._table_names.items()}
        self.opt = torch.optim.Adam(list(self.w.values()), lr=1e-3, eps=1e-7, capturable=True)
        self.l2 = float(m.l2_reg_embedding or 0)

    def tower(self, tw, prefix, x):
        class L:  # torch_tower reads m.tables and each layer's kernel / bias
            pass
        shim, twv = L(), L()
        shim.tables = self.tables
        twv.sparse_cols, twv.varlen_cols, twv.dnn = tw.sparse_cols, tw.varlen_cols, L()
        twv.dnn.layers = []
        for i in range(len(tw.dnn.layers)):
            lay = L()
            lay.kernel, lay.bias = self.w[f"{prefix}/kernel{i}"], self.w[f"{prefix}/bias{i}"]
            twv.dnn.layers.append(lay)
        return torch_tower(shim, twv, x)

    def __call__(self, x):
        m = self.m
        u, v = self.tower(m.user_tower, "dnn", x), self.tower(m.item_tower, "dnn_1", x)
        z = (u / m.temperature) @ v.t() - m.softmax.logq[x["movie_id"]].unsqueeze(0)
        loss = (torch.logsumexp(z, dim=1) - torch.diagonal(z)).mean()
        loss = loss + self.l2 * sum((t * t).sum() for t in self.tables.values())
        self.opt.zero_grad(set_to_none=False)
        loss.backward()
        self.opt.step()
        return loss


def time_batch(m, ref, gen, B, dev):
    x, n_valid = make_inputs(B, gen, dev)
    parts = {"train_step": lambda: m.train_step(x, check_ids=False), "torch": lambda: ref(x)}
    first = float(m.gradients(x, check_ids=False)[1].mean())
    # every replay must hold exactly the REPS steps the times are divided by: count the calls under capture
    calls = {n: 0 for n in parts}

    def counted(n, fn):
        def call():
            calls[n] += 1
            return fn()
        return call

    runners = {n: runner(counted(n, fn), REPS) for n, fn in parts.items()}
    for n, (_, mode) in runners.items():   # runner: 3 warm-up calls, 1 on the side stream, then the captured ones
        captured = calls[n] - 4
        assert mode != "graph" or captured == REPS, f"{n}: {captured} steps captured, times divided by {REPS}"
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
    last = float(m.gradients(x, check_ids=False)[1].mean())
    # algorithmic bytes of one step per sample: the forward's ids, lengths and rows, the same rows' gradients' reads
    # of dx (once per valid position), and Adam's 7 accesses (w, g, m, v read; w, m, v written) of every parameter
    isz = x["hist_movie_id"].element_size()
    n_param = sum(p.numel() for k, p in m.keras_weights().items())
    per_sample = (7 * isz + x["hist_len"].element_size() + 5 * 16 * 4 + 2 * 32 * 4) + n_valid / B * 2 * (isz + 2 * 32 * 4)
    return {
        "workload": f"DSSM demo towers, ml-1m vocabularies, T {T}, in-batch softmax t {m.temperature}, Adam, B {B}",
        "median_us": {n: round(v, 2) for n, v in med.items()},
        "min_us": {n: round(v, 2) for n, v in lo.items()},
        "max_us": {n: round(v, 2) for n, v in hi.items()},
        "mode": {n: r[1] for n, r in runners.items()},
        "steps_per_replay": REPS,
        "train_step_over_torch": round(med["train_step"] / med["torch"], 3),
        "gap_us_min_torch_minus_max_train_step": round(lo["torch"] - hi["train_step"], 2),
        "train_step_faster_than_torch": hi["train_step"] < lo["torch"],
        "torch_faster_than_train_step": hi["torch"] < lo["train_step"],
        "input_bytes_per_sample": round(per_sample, 1),
        "adam_bytes_per_step": 7 * 4 * n_param,
        "parameters": n_param,
        "mean_length": round(n_valid / B, 2),
        "mean_loss_before_after": [round(first, 4), round(last, 4)]}


def main():
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda")
    m, gen = build_model(dev)
    if os.environ.get("DSSM_TRAIN_PROFILE") == "1":
        x, _ = make_inputs(BATCHES[0], gen, dev)
        for _ in range(5):
            m.train_step(x, check_ids=False)
        torch.cuda.synchronize()
        return
    ref = TorchStep(m)
    res = {f"B{B}": time_batch(m, ref, gen, B, dev) for B in BATCHES}
    line = json.dumps({"script": "scripts/time_dssm_train.py", "reps": REPS, "rounds": ROUNDS, **res})
    print(line)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
