#!/usr/bin/env python3
"""The SPA exit gate's statistic on the CPU oracle.

The register decoder's checked scan of iteration k counts the rows whose
parity misses the target syndrome (c_k: the totals after k iterations).  A
converging frame leaves at the scan that counts 0.  The gate runs a
parity-only pass before scan k when c_{k-1} <= theta; this script decodes the
bench's own trials with the oracle's per-iteration trace and prints, for each
theta, the passes per frame and the share of exits the gate catches (without
and with a limit on the gated passes a frame may lose), and the
smallest theta that catches >= 99 % of the converging frames' exits.

  python tools/exit_gate_stats.py [--workload c2] [--frames 512] [--source oracle|gpu]

--source gpu takes the counts from the GPU instead: Graph.decode_trace(...).unsat
on a frame-per-lane graph, one batch for all the frames (the same numbers; the
oracle decodes one frame at a time).
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from conftest import load_fixture  # noqa: E402
from oracle import pyoracle as P  # noqa: E402

# fixture, QBER, simulation seed: bench.py's WORKLOADS / SIMULATION_SEEDS
CASES = {"c2": ("c2_n10240_m2201.alist", 0.0215, 1022025), "c1": ("c1_n1024_m220.alist", 0.013, 9012025)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="c2", choices=sorted(CASES))
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--max-iterations", type=int, default=50)
    ap.add_argument("--misses", type=int, default=8,
                    help="a limit on the gated passes a frame may lose (measured, not built: DESIGN.md §3.3)")
    ap.add_argument("--source", default="oracle", choices=["oracle", "gpu"],
                    help="where the per-iteration counts come from: the CPU oracle's posteriors, or the GPU trace")
    args = ap.parse_args()
    fx, qber, seed = CASES[args.workload]
    H = load_fixture(fx)
    O = P.Oracle(H)
    p = O.params(0, args.max_iterations, True, 100.0, 0.0, 0.0)
    rp = np.asarray(H.row_ptr[:-1], np.int64)
    ci = np.asarray(H.col_idx, np.int64)
    assert (np.diff(np.asarray(H.row_ptr)) > 0).all()
    before_exit, tracks, iters, oks = [], [], [], []

    def trials():
        for sd in P.trial_seeds(seed, args.frames):
            a, b, q = P.trial(H.n, qber, int(sd))
            lp = np.log((1.0 - q) / q)
            yield np.where(b != 0, -lp, lp), H.syndrome(a[None, :])[0]

    def oracle_counts():
        """-> per frame (iterations, ok, c): c[j] = the count of scan j + 1 (totals after j + 1 iterations)"""
        for llr, s in trials():
            _, it, ok, _, tr = O.decode(p, llr, s, trace=True)
            z = (tr[:it] <= 0.0).astype(np.int64)
            yield it, ok, ((np.add.reduceat(z[:, ci], rp, axis=1) & 1) != s[None, :]).sum(axis=1)

    def gpu_counts():
        import qkd_ldpc_v_amd as Q

        llr, synd = (np.stack(x) for x in zip(*trials()))
        out = Q.Graph(H, layout="frame_per_lane").decode_trace(Q.Params(Q.SPA, args.max_iterations, True, 100.0),
                                                               llr, synd)
        assert np.array_equal(out.rows, out.iterations)
        for it, ok, u in zip(out.iterations, out.synd_ok, out.unsat):
            yield int(it), bool(ok), u[:int(it)].astype(np.int64)

    for it, ok, c in (gpu_counts() if args.source == "gpu" else oracle_counts()):
        assert (c[-1] == 0) == bool(ok)
        iters.append(it)
        oks.append(bool(ok))
        # gate decisions: before scan k = 2 .. it (converging) or 2 .. cap - 1 (the cap's pass always runs);
        # the decision before scan k reads c[k - 2]
        last = it if ok else it - 1
        tracks.append(c[:max(last - 1, 0)])
        if ok:
            before_exit.append(int(c[it - 2]) if it >= 2 else -1)
    be = np.array(before_exit)
    conv = len(be)

    def run(theta, misses):
        """-> (passes per frame, passes per failing frame, share of exits caught) of the
        gate at theta; misses: the gated passes a frame may lose, i.e. that find
        a row off (None: no limit, as the kernel runs)."""
        passes = fpasses = caught = 0
        for t, ok in zip(tracks, oks):
            lost = 0
            for j, cj in enumerate(t):
                if cj <= theta and (misses is None or lost < misses):
                    passes += 1
                    fpasses += 0 if ok else 1
                    if ok and j == len(t) - 1:
                        caught += 1
                    else:
                        lost += 1
        nf = max(1, len(oks) - conv)
        return round(passes / len(tracks), 3), round(fpasses / nf, 2), round(caught / conv, 4)

    rows = []
    for theta in (8, 16, 24, 32, 40, 48, 54, 56, 64, 80, 96, 128, 1 << 30):
        p0, f0, c0 = run(theta, None)
        p1, f1, c1 = run(theta, args.misses)
        rows.append({"theta": theta, "unlimited": {"passes_per_frame": p0, "per_failing_frame": f0, "exits_caught": c0},
                     "limited": {"passes_per_frame": p1, "per_failing_frame": f1, "exits_caught": c1}})
    srt = np.sort(np.where(be < 0, 1 << 30, be))
    need = int(np.ceil(0.99 * conv))
    theta99 = int(srt[need - 1])
    print(json.dumps({
        "workload": args.workload, "frames": args.frames, "converging": conv, "m": int(H.m),
        "mean_iterations": float(np.mean(iters)),
        "count_before_exit": {"min": int(be[be >= 0].min()), "median": float(np.median(be[be >= 0])),
                              "p99": int(np.percentile(be[be >= 0], 99)), "max": int(be.max()),
                              "exits_at_iteration_1": int((be < 0).sum())},
        "smallest_theta_for_99pct": theta99, "misses": args.misses, "table": rows}))


if __name__ == "__main__":
    main()
