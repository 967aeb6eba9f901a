"""Cost of Bob's selection (qldpc_select_positions_device) against the decode of
the same symmetric round, for 512 failed frames of the C2 graph (n = 10240):
count 20 and 200 on the posteriors the failed decode left, and the positions
round of those 512 frames with 20 positions pinned (INTEGRATION.md §7,
"Symmetric rounds").  Needs the GPU.  Writes profiles/blind/select_cost.json."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import qkd_ldpc_v_amd as Q  # noqa: E402
from conftest import load_fixture  # noqa: E402

FAILED, CAP, QBER, CHUNK = 512, 20, 0.032, 1024
H = load_fixture("c2_n10240_m2201.alist")
g = Q.Graph(H)
par = Q.Params(Q.SPA, CAP, True, 100.0)


def cu(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


# frames until 512 of them have failed one-shot (no plan: every position is a key position)
keys_a, keys_b, syns, posts = [], [], [], []
lp, have, seed, drawn = None, 0, 50, 0
while have < FAILED:
    a, b, q = Q.bsc_frames(H.n, QBER, CHUNK, seed=seed)
    seed, drawn, lp = seed + 1, drawn + CHUNK, Q.log_p(q)
    syn = g.syndrome(a)
    out = g.reconcile(par, b, lp, syn, posterior=True)
    bad = np.flatnonzero(out.synd_ok == 0)[:FAILED - have]
    if bad.size == 0 and drawn >= 64 * CHUNK:
        raise SystemExit(f"no frame fails at QBER {QBER}")
    keys_a.append(a[bad]); keys_b.append(b[bad]); syns.append(syn[bad]); posts.append(out.posterior[bad])
    have += bad.size
alice, bob, syn, post = (np.concatenate(x) for x in (keys_a, keys_b, syns, posts))
d_post, d_key, d_lp, d_syn = cu(post), cu(bob), cu(np.full(FAILED, lp)), cu(syn)
d_list = cu(np.arange(FAILED, dtype=np.int32))
d_pos = torch.full((FAILED, 256), -1, dtype=torch.int32, device="cuda")
g.select_positions_device(d_post, d_list, 0, 20, d_pos)
torch.cuda.synchronize()
pos = d_pos.cpu().numpy()
u = post.view(np.uint64) & np.uint64(0x7FFFFFFFFFFFFFFF)
for f in (0, FAILED - 1):  # the selection is numpy's
    assert np.array_equal(pos[f, :20], np.lexsort((np.arange(H.n), u[f]))[:20])
d_vals = torch.empty((FAILED, 20), dtype=torch.uint8, device="cuda")
g.disclose_positions_device(cu(alice), d_list, d_pos, 0, 20, d_vals)
d_pos20 = d_pos.clone()
bits = torch.empty((FAILED, H.n), dtype=torch.uint8, device="cuda")
it = torch.empty(FAILED, dtype=torch.int32, device="cuda")
ok = torch.empty(FAILED, dtype=torch.uint8, device="cuda")


def select20():
    g.select_positions_device(d_post, d_list, 0, 20, d_pos)


def select200():
    g.select_positions_device(d_post, d_list, 0, 200, d_pos)


def round20():  # frames build + decode + scatter of the 512 frames, 20 positions pinned
    g.reconcile_positions_round_device(par, d_key, d_lp, d_syn, d_list, 20, d_pos20, d_vals, bits, it, ok)


calls = {"select_count_20": select20, "select_count_200": select200, "positions_round_decode": round20}
for f in calls.values():
    for _ in range(5):
        f()
torch.cuda.synchronize()
REPS, WINDOWS = 20, 7
ms = {k: [] for k in calls}
for _ in range(WINDOWS):
    for k, f in calls.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(REPS):
            f()
        torch.cuda.synchronize()
        ms[k].append((time.perf_counter() - t0) * 1e3 / REPS)
med = {k: float(np.median(v)) for k, v in ms.items()}
res = {"code": "C2", "n": H.n, "failed_frames": FAILED, "frames_drawn": drawn, "qber": QBER, "cap": CAP,
       "decoded_in_round": int(ok.cpu().numpy().sum()), "mean_iterations_round": float(it.cpu().numpy().mean()),
       "ms_per_call_median": med, "ms_per_call_min_max": {k: [float(min(v)), float(max(v))] for k, v in ms.items()},
       "select_over_round": {"count_20": med["select_count_20"] / med["positions_round_decode"],
                             "count_200": med["select_count_200"] / med["positions_round_decode"]},
       "select_bytes_per_frame_one_pass": 8 * H.n}
OUT = os.path.join(ROOT, "profiles", "blind")
os.makedirs(OUT, exist_ok=True)
with open(os.path.join(OUT, "select_cost.json"), "w") as fh:
    json.dump(res, fh, indent=1)
print(json.dumps(res))
