"""Timing of the AFM training step's fused launch (rs_afm_train_fwd) at
B 4096, F 26, k 16 (26 fields x 1e6 rows: the table of bench.py --config afm),
in the same process on the same weights:

  one_launch[mode]  : rs_afm_train_fwd ('att', 'avg', 'max'): pooled, prob, g,
                      loss and the [B, F*k] row gradients in ONE launch;
  composed[mode]    : the same quantities from the entries that existed before
                      it ('att' and 'avg'; 'max' has no such composition):
                      rs_embed_gather (rows to memory), rs_embed_pair_pool_fwd
                      with its head (one sigmoid), torch element-wise ops for
                      prob / loss / g / g w, rs_bi_interaction_bwd;
  train_step[mode]  : the whole AFM.train_step(check_ids=False).

Every call of a timed window takes the next of NB id batches, so the rows come
from HBM as in training and not from a cache warmed by the call before.  Each
variant is replayed from a captured graph (REPS calls per replay; eager calls
if a capture fails), the variants alternate over ROUNDS rounds, times come
from device events and the medians are reported with each variant's min and
max over the rounds.  Writes one JSON line to profiles/afm_train_timing.jsonl
(--out) and prints it."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import recommender_system_amd as rs  # noqa: E402
from recommender_system_amd import _lib  # noqa: E402
from recommender_system_amd._lib import call, ptr  # noqa: E402

REPS = int(os.environ.get("AFM_REPS", "256"))
STEP_REPS = int(os.environ.get("AFM_STEP_REPS", "16"))
ROUNDS = int(os.environ.get("AFM_ROUNDS", "9"))
NB = int(os.environ.get("AFM_BATCHES", "64"))
B = int(os.environ.get("AFM_B", "4096"))
F = int(os.environ.get("AFM_F", "26"))
K = int(os.environ.get("AFM_K", "16"))
V = int(os.environ.get("AFM_V", "1000000"))
MODES = {"att": 0, "avg": 1, "max": 2}


def runner(fn, reps):
    """fn(i), i = 0..reps-1, replayed from a captured graph ('graph'), or
    called eagerly ('eager') when the capture fails."""
    for i in range(3):
        fn(i)
    torch.cuda.synchronize()
    try:
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s):
            fn(0)
            torch.cuda.synchronize()
            with torch.cuda.graph(g, stream=s):
                for i in range(reps):
                    fn(i)
        torch.cuda.synchronize()
        return g.replay, "graph"
    except Exception as ex:  # noqa: BLE001
        torch.cuda.synchronize()
        print(f"capture failed ({type(ex).__name__}: {ex}); eager timing", file=sys.stderr)

        def eager():
            for i in range(reps):
                fn(i)
        return eager, "eager"


def main():
    assert torch.cuda.is_available(), "needs an MI355X"
    out_path = os.path.join(ROOT, "profiles", "afm_train_timing.jsonl")
    if "--out" in sys.argv:
        out_path = sys.argv[sys.argv.index("--out") + 1]
    dev = torch.device("cuda")
    cols = [[], [{"feat": f"C{i + 1}", "feat_onehot_dim": V, "embed_dim": K} for i in range(F)]]
    models = {mode: rs.AFM(cols, mode, device=dev, seed=0) for mode in MODES}
    gen = torch.Generator(device="cpu").manual_seed(1)
    ids = torch.randint(0, V, (NB, B, F), generator=gen, dtype=torch.int32).to(dev)
    labels = torch.randint(0, 2, (B,), generator=gen).to(torch.float32).to(dev)
    dense = torch.zeros(B, 0, dtype=torch.float32, device=dev)
    for m in models.values():  # O(1) logits, as test_interactions scales the Keras inits
        with torch.no_grad():
            m.afm_layer.embed_layer.table.mul_(10.0)
            m.afm_layer.output_layer.kernel.mul_(3.0)
        m._weights_changed()
    L = models["att"].afm_layer
    e, head = L.embed_layer, L.output_layer
    emp = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
    pooled, prob, g, loss, de = emp(B, K), emp(B), emp(B), emp(B), emp(B, F * K)
    rows, s1, pooled2, de2 = emp(B, F * K), emp(B, 1), emp(B, K), emp(B, F * K)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    st = _lib.stream

    def one_launch(mode):
        def fn(i):
            x = ids[i % NB]
            call("rs_afm_train_fwd", ptr(x), _lib.ID_I32, F, ptr(e.table), ptr(e.field_offsets), ptr(e.field_vocab),
                 F, K, MODES[mode], ptr(head.kernel), ptr(head.bias), 2, ptr(labels), B, ptr(pooled), K, ptr(prob),
                 ptr(g), ptr(loss), ptr(de), F * K, ptr(flag), st())
            return pooled, prob, g, loss, de
        return fn

    def composed(mode):
        scale = 1.0 / (F * (F - 1) // 2) if mode == "avg" else 1.0
        w = head.kernel.reshape(1, K)

        def fn(i):
            x = ids[i % NB]
            call("rs_embed_gather", ptr(x), _lib.ID_I32, F, None, 0, 0, ptr(e.table), ptr(e.field_offsets),
                 ptr(e.field_vocab), F, K, ptr(rows), F * K, B, ptr(flag), st())
            call("rs_embed_pair_pool_fwd", ptr(x), _lib.ID_I32, F, ptr(e.table), ptr(e.field_offsets),
                 ptr(e.field_vocab), F, K, MODES[mode], None, 0, 0, ptr(pooled2), K, 0, ptr(head.kernel),
                 ptr(head.bias), 1, ptr(s1), B, ptr(flag), st())
            s = s1.view(B)
            p = torch.sigmoid(s)
            ls = s - s * labels + torch.log1p(torch.exp(-s))
            gg = (p - labels) * s * (1 - s) / B
            dbi = (gg * scale).view(B, 1) * w
            call("rs_bi_interaction_bwd", ptr(rows), F * K, ptr(dbi), K, F, K, B, ptr(de2), F * K, st())
            return pooled2, p, gg, ls, de2
        return fn

    def train_step(mode):
        m = models[mode]

        def fn(i):
            return m.train_step((dense, ids[i % NB]), labels, lr=0.01, return_loss=True, check_ids=False)
        return fn

    parts, reps = {}, {}
    for mode in MODES:
        parts[f"one_launch[{mode}]"], reps[f"one_launch[{mode}]"] = one_launch(mode), REPS
    for mode in ("att", "avg"):
        parts[f"composed[{mode}]"], reps[f"composed[{mode}]"] = composed(mode), REPS
    for mode in MODES:
        parts[f"train_step[{mode}]"], reps[f"train_step[{mode}]"] = train_step(mode), STEP_REPS

    agree = {}
    for mode in ("att", "avg"):  # the two ways compute the same quantities
        a = [t.clone() for t in one_launch(mode)(0)]
        b = [t.clone() for t in composed(mode)(0)]
        torch.cuda.synchronize()
        agree[mode] = {n: float((x - y).abs().max() / y.abs().max().clamp_min(1e-30))
                       for n, x, y in zip(("pooled", "prob", "g", "loss", "drows"), a, b)}

    runners = {n: runner(fn, reps[n]) for n, fn in parts.items()}
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
            times[n].append(e0.elapsed_time(e1) * 1e3 / reps[n])
    med = {n: float(np.median(v)) for n, v in times.items()}
    res = {
        "script": "scripts/time_afm_train.py", "reps": REPS, "step_reps": STEP_REPS, "rounds": ROUNDS,
        "id_batches": NB,
        "workload": f"AFM train B {B} F {F} k {K} vocab {V} per field",
        "median_us": {n: round(v, 2) for n, v in med.items()},
        "min_us": {n: round(float(np.min(v)), 2) for n, v in times.items()},
        "max_us": {n: round(float(np.max(v)), 2) for n, v in times.items()},
        "mode": {n: r[1] for n, r in runners.items()},
        "one_launch_over_composed": {m: round(med[f"one_launch[{m}]"] / med[f"composed[{m}]"], 3)
                                     for m in ("att", "avg")},
        # the margin of the comparison: the composition's own min-to-max spread over the rounds
        "composed_spread_us": {m: round(float(np.max(times[f"composed[{m}]"]) - np.min(times[f"composed[{m}]"])), 2)
                               for m in ("att", "avg")},
        "bytes_per_sample": {"rows_read": F * K * 4, "ids_read": F * 4, "drows_written": F * K * 4,
                             "pooled_prob_g_loss_written": K * 4 + 12},
        "max_rel_diff_one_launch_vs_composed": agree}
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
