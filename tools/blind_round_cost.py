"""Cost of one disclosure round (qldpc_reconcile_round_device) against
qldpc_decode_batch_device on the same pinned LLRs already compact, and against
qldpc_reconcile_batch_device on the same number of frames (DESIGN.md,
"Disclosure rounds").  Needs the GPU.  Writes profiles/blind/round_cost.json."""
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
from test_gpu_blind import PUNCT, SHORT, pinned_llr  # noqa: E402
from test_gpu_parties import np_extend, np_llr  # noqa: E402

BATCH, CAP = 4096, 20
H = load_fixture("c1_n1024_m220.alist")
g = Q.Graph(H)
plan = g.rate_plan(PUNCT, SHORT)
par = Q.Params(Q.SPA, CAP, True, 100.0)
a, b, q = Q.bsc_frames(H.n, 0.016, BATCH, seed=11)
fill = np.random.Generator(np.random.PCG64(3)).integers(0, 2, (BATCH, 60)).astype(np.uint8)
lp = Q.log_p(q)
syn = H.syndrome(np_extend(a, fill, PUNCT, SHORT))


def cu(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def outs(nb):
    return (torch.empty((nb, H.n), dtype=torch.uint8, device="cuda"), torch.empty(nb, dtype=torch.int32, device="cuda"),
            torch.empty(nb, dtype=torch.uint8, device="cuda"))


d_key, d_lp, d_syn = cu(b), cu(np.full(BATCH, lp)), cu(syn)
bits, it, ok = outs(BATCH)
g.reconcile_device(par, d_key, d_lp, d_syn, bits, it, ok, plan=plan)
lst = torch.empty(BATCH, dtype=torch.int32, device="cuda")
cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
g.failed_frames_device(ok, lst, cnt)
torch.cuda.synchronize()
nf = int(cnt.cpu()[0])
failed = lst[:nf].cpu().numpy()
assert np.array_equal(failed, np.flatnonzero(ok.cpu().numpy() == 0))
disc = np.arange(20, dtype=np.int32)
d_disc, d_vals = cu(disc), cu(fill[failed][:, disc])
# the same frames as a batch of their own
c_key, c_lp, c_syn = cu(b[failed]), cu(np.full(nf, lp)), cu(syn[failed])
c_llr = cu(pinned_llr(np_llr(b, lp, PUNCT, SHORT), PUNCT, fill, failed, disc))
cb, ci, co = outs(nf)
rb, ri, ro = bits.clone(), it.clone(), ok.clone()


def round_call():
    g.reconcile_round_device(par, d_key, d_lp, d_syn, plan, lst, d_disc, d_vals, rb, ri, ro, n_list=nf)


def reconcile_call():  # (the one-shot entry on nf frames: no pins, palette path)
    g.reconcile_device(par, c_key, c_lp, c_syn, cb, ci, co, plan=plan)


def decode_call():  # (the round's decode alone: the pinned LLRs, already compact)
    g.decode_device(par, c_llr, c_syn, cb, ci, co)


calls = {"round": round_call, "reconcile_same_count": reconcile_call, "decode_pinned_llr": decode_call}
for f in calls.values():
    for _ in range(5):
        f()
torch.cuda.synchronize()
# the round equals the decode of the pinned LLRs
decode_call()
round_call()
torch.cuda.synchronize()
assert np.array_equal(rb.cpu().numpy()[failed], cb.cpu().numpy()) and np.array_equal(ri.cpu().numpy()[failed], ci.cpu().numpy())
REPS, WINDOWS = 50, 9
ms = {k: [] for k in calls}
for _ in range(WINDOWS):
    for k, f in calls.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(REPS):
            f()
        torch.cuda.synchronize()
        ms[k].append((time.perf_counter() - t0) * 1e3 / REPS)
res = {"code": "C1", "batch": BATCH, "frames_in_round": nf, "cap": CAP, "n_disc": 20, "decoded_in_round": int(ro.cpu().numpy()[failed].sum()),
       "mean_iterations_round": float(ri.cpu().numpy()[failed].mean()),
       "ms_per_call_median": {k: float(np.median(v)) for k, v in ms.items()},
       "ms_per_call_min_max": {k: [float(min(v)), float(max(v))] for k, v in ms.items()}}
OUT = os.path.join(ROOT, "profiles", "blind")
os.makedirs(OUT, exist_ok=True)
with open(os.path.join(OUT, "round_cost.json"), "w") as fh:
    json.dump(res, fh, indent=1)
print(json.dumps(res))
