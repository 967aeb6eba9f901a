"""Cost of the error estimate (qldpc_estimate_qber_device: the syndrome-weight
kernel and the solve, two launches) and of qldpc_corrected_errors_device
against the steps beside them, for 4096 frames of the C2 graph (n = 10240) at
QBER 0.0215: Alice's qldpc_syndrome_batch_device of the same batch (the existing
kernel with the same memory traffic, less the m syndrome bytes the weight kernel
reads) and Bob's qldpc_reconcile_batch_device, SPA capped at 50 iterations (the
step the estimate feeds).  Without a plan, and with 100 punctured and 100
shortened positions.  Needs the GPU.  Writes
profiles/estimate/cost.json."""
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

FRAMES, CAP, QBER = 4096, 50, 0.0215
REPS, WINDOWS = 20, 7
H = load_fixture("c2_n10240_m2201.alist")
g = Q.Graph(H)
par = Q.Params(Q.SPA, CAP, True, 100.0)


def cu(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


# The solve was built both ways and measured once, in this script's setup, before
# the slower form was removed: as the tail of the weight kernel (thread 0 of
# each frame's workgroup solves) against the second launch with one thread per
# frame.  ms per call, medians of 7 windows of 20 calls, same bits either way.
FUSED_EXPERIMENT = {
    "note": "fused: the solve as the tail of the weight kernel, one lane per frame; two_launch: what is built "
            "(both measured before the weight kernel's loads were reordered, which took 6.5 us off either form)",
    "no_plan": {"fused": 0.12701, "two_launch": 0.10635, "weight_only": 0.07194},
    "plan_100_100": {"fused": 0.18590, "two_launch": 0.15605, "weight_only": 0.11508},
}


def measure(calls):
    for f in calls.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in calls}
    for _ in range(WINDOWS):
        for k, f in calls.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(REPS):
                f()
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3 / REPS)
    return ({k: float(np.median(v)) for k, v in ms.items()},
            {k: [float(min(v)), float(max(v))] for k, v in ms.items()})


def case(plan, punct, short):
    alice, bob, q = Q.bsc_frames(H.n, QBER, FRAMES, seed=1810)
    fill = np.random.Generator(np.random.PCG64(5)).integers(0, 2, (FRAMES, max(1, punct.size))).astype(np.uint8)
    d_alice, d_bob, d_fill = cu(alice), cu(bob), cu(fill)
    d_syn = torch.empty((FRAMES, H.m), dtype=torch.uint8, device="cuda")
    g.syndrome_device(d_alice, d_syn, plan, d_fill if punct.size else None)
    d_w = torch.empty(FRAMES, dtype=torch.int32, device="cuda")
    d_q = torch.empty(FRAMES, dtype=torch.float64, device="cuda")
    d_lp = torch.empty(FRAMES, dtype=torch.float64, device="cuda")
    d_err = torch.empty(FRAMES, dtype=torch.int32, device="cuda")
    bits = torch.empty((FRAMES, H.n), dtype=torch.uint8, device="cuda")
    it = torch.empty(FRAMES, dtype=torch.int32, device="cuda")
    ok = torch.empty(FRAMES, dtype=torch.uint8, device="cuda")
    g.estimate_qber_device(d_bob, d_syn, d_w, d_q, d_lp, plan=plan)
    g.reconcile_device(par, d_bob, d_lp, d_syn, bits, it, ok, plan=plan)
    torch.cuda.synchronize()
    calls = {
        "alice_syndrome": lambda: g.syndrome_device(d_alice, d_syn, plan, d_fill if punct.size else None),
        "estimate_weight_only": lambda: g.estimate_qber_device(d_bob, d_syn, d_w, plan=plan),
        "estimate_weight_and_solve": lambda: g.estimate_qber_device(d_bob, d_syn, d_w, d_q, d_lp, plan=plan),
        "corrected_errors": lambda: g.corrected_errors_device(d_bob, bits, d_err, plan=plan),
        "reconcile_spa50": lambda: g.reconcile_device(par, d_bob, d_lp, d_syn, bits, it, ok, plan=plan),
    }
    med, span = measure(calls)
    qh = d_q.cpu().numpy()
    deg, rows = g.estimate_classes(plan)
    return {"punctured": int(punct.size), "shortened": int(short.size), "informative_rows": int(rows.sum()),
            "classes": {"degree": deg.tolist(), "rows": rows.tolist()},
            "true_qber": float(q), "estimate_mean": float(qh.mean()), "estimate_std": float(qh.std()),
            "decoded": int(ok.cpu().numpy().sum()), "mean_iterations": float(it.cpu().numpy().mean()),
            "mean_corrected_errors": float(d_err.cpu().numpy().mean()),
            "ms_per_call_median": med, "ms_per_call_min_max": span,
            "solve_ms": med["estimate_weight_and_solve"] - med["estimate_weight_only"],
            "weight_over_alice_syndrome": med["estimate_weight_only"] / med["alice_syndrome"],
            "estimate_over_reconcile": med["estimate_weight_and_solve"] / med["reconcile_spa50"],
            "corrected_errors_over_reconcile": med["corrected_errors"] / med["reconcile_spa50"]}


pos = np.random.Generator(np.random.PCG64(1810)).permutation(H.n)[:200]
punct, short = np.sort(pos[:100]).astype(np.int32), np.sort(pos[100:]).astype(np.int32)
none = np.empty(0, np.int32)
res = {"code": "C2", "n": H.n, "m": H.m, "frames": FRAMES, "qber": QBER, "cap": CAP, "windows": WINDOWS,
       "calls_per_window": REPS, "solve": "a second launch, one thread per frame", "fused_solve_experiment": FUSED_EXPERIMENT,
       "no_plan": case(None, none, none), "plan_100_100": case(g.rate_plan(punct, short), punct, short)}
OUT = os.path.join(ROOT, "profiles", "estimate")
os.makedirs(OUT, exist_ok=True)
with open(os.path.join(OUT, "cost.json"), "w") as fh:
    json.dump(res, fh, indent=1)
print(json.dumps(res))
