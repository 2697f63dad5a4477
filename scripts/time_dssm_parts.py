"""Where the fused DSSM user tower's time goes: rs_dssm_tower_fwd timed alone
(DSSM.user_embedding from a captured graph, as scripts/time_dssm.py times it)
on variants of the demo's user tower — all pieces or the profile ids / the
sequences alone, with and without the three layers — at B (environment, 256).
Prints one JSON line of medians in µs per call; each includes the fill of the
error flag, timed alone as ``fill_only``."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import recommender_system_amd as rs  # noqa: E402
import time_dssm as td  # noqa: E402

S, V = rs.SparseFeat, rs.VarLenSparseFeat
dev = torch.device("cuda")
B = int(os.environ.get("B", "256"))
gen = torch.Generator(device="cpu").manual_seed(1)
x, _ = td.make_inputs(B, gen, dev)
prof = [S(n, td.VOCAB[n], 16) for n in td.PROFILE]
seqs = [V(S("hist_movie_id", td.VOCAB["movie_id"], 32, embedding_name="movie_id"), 50, "mean", "hist_len"),
        V(S("hist_genres", td.VOCAB["genres"], 32, embedding_name="genres"), 50, "mean", "hist_len")]
variants = {
    "full_3layers": (prof + seqs, (128, 64, 32)),
    "full_0layers": (prof + seqs, ()),
    "profile_3layers": (prof, (128, 64, 32)),
    "profile_0layers": (prof, ()),
    "seq_0layers": (seqs, ()),
    "oneseq_0layers": (seqs[:1], ()),
}
res = {}
for name, (cols, hidden) in variants.items():
    width = hidden[-1] if hidden else sum(c.embedding_dim for c in cols)
    m = rs.DSSM(cols, [S("item", 10, width)], hidden, (), loss_type="logistic", device=dev, seed=0)
    assert m.user_tower.fused_ok()
    fn = lambda m=m: m.user_embedding(x, check_ids=False)
    run, mode = td.runner(fn)
    ts = []
    for _ in range(7):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3 / td.REPS)
    res[name] = round(float(np.median(ts)), 2)
# the error flag's fill alone
fn = lambda: torch.zeros(1, dtype=torch.int32, device=dev)
run, mode = td.runner(fn)
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
run()
e1.record()
torch.cuda.synchronize()
res["fill_only"] = round(e0.elapsed_time(e1) * 1e3 / td.REPS, 2)
print(json.dumps({"B": B, **res}))
