"""What the estimate buys the decode: 256 frames of the C2 graph (n = 10240)
whose true QBER is drawn per frame, uniform in [0.015, 0.028], decoded by the
CPU oracle (SPA capped at 50 iterations) four times, with log_p from
  (a) the batch's mean QBER, the same for every frame;
  (b) the pooled estimate (one root from the sum of the syndrome weights);
  (c) the per-frame estimate;
  (d) each frame's true QBER.
FER and mean iterations per arm.  No GPU: the weights are
numpy's (tests/estimate_ref.py), the roots the product's host solver
(qldpc_qber_from_weight on a host-only graph).  Writes
profiles/estimate/benefit.json."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import estimate_ref as R  # noqa: E402
import qkd_ldpc_v_amd as Q  # noqa: E402
from conftest import load_fixture  # noqa: E402
from oracle.pyoracle import Oracle  # noqa: E402

FRAMES, CAP, Q_LO, Q_HI, SEED = 256, 50, 0.015, 0.028, 1810
Q_MIN, Q_MAX = 1e-4, 0.25
H = load_fixture("c2_n10240_m2201.alist")
g = Q.Graph(H, host_only=True)
rng = np.random.Generator(np.random.PCG64(SEED))
alice = rng.integers(0, 2, (FRAMES, H.n), dtype=np.uint8)
flips = np.floor(H.n * rng.uniform(Q_LO, Q_HI, FRAMES)).astype(np.int64)
bob = alice.copy()
for f in range(FRAMES):
    bob[f, rng.choice(H.n, int(flips[f]), replace=False)] ^= 1
q_true = flips / H.n
syn = H.syndrome(alice)
w = R.weights(R.dense(H), bob, syn)
q_frame, lp_frame = g.qber_from_weight(w, None, Q_MIN, Q_MAX)
q_pool, lp_pool = g.qber_from_weight([int(w.sum())], None, Q_MIN, Q_MAX, frames_per_weight=FRAMES)
arms = {
    "a_mean_qber": np.full(FRAMES, R.log_p(float(q_true.mean()))),
    "b_pooled_estimate": np.full(FRAMES, lp_pool[0]),
    "c_per_frame_estimate": lp_frame,
    "d_true_qber": np.array([R.log_p(float(x)) for x in q_true]),
}
O = Oracle(H)
par = O.params(Q.SPA, CAP, True, 100.0)
res = {"code": "C2", "n": H.n, "m": H.m, "frames": FRAMES, "cap": CAP, "qber_range": [Q_LO, Q_HI], "seed": SEED,
       "mean_true_qber": float(q_true.mean()), "pooled_estimate": float(q_pool[0]),
       "per_frame_estimate_error_std": float((q_frame - q_true).std()),
       "per_frame_estimate_error_mean": float((q_frame - q_true).mean()), "arms": {}}
for name, lp in arms.items():
    llr = np.where(bob != 0, -lp[:, None], lp[:, None])
    bits, it, ok, _ = O.decode_batch(par, llr, syn, threads=min(8, os.cpu_count() or 1), posterior=False)
    wrong = (bits != alice).any(axis=1)
    res["arms"][name] = {"fer": float(wrong.mean()), "frames_failed": int(wrong.sum()),
                         "syndrome_failed": int((ok == 0).sum()), "mean_iterations": float(it.mean())}
    print(name, res["arms"][name], flush=True)
d = res["arms"]["d_true_qber"]
res["distance_to_true_qber_arm"] = {
    k: {"fer": v["fer"] - d["fer"], "mean_iterations": v["mean_iterations"] - d["mean_iterations"]}
    for k, v in res["arms"].items() if k != "d_true_qber"}
OUT = os.path.join(ROOT, "profiles", "estimate")
os.makedirs(OUT, exist_ok=True)
with open(os.path.join(OUT, "benefit.json"), "w") as fh:
    json.dump(res, fh, indent=1)
print(json.dumps(res))
