#!/usr/bin/env python3
"""Wall time of Graph.reconcile (host entry: Bob's key bytes in) against
Graph.decode (8-byte LLRs in) on the same frames: the C2 operating point
(n = 10240, SPA, 50 iterations, QBER 2.15 %), 4096 frames, one GPU.  The two
alternate in one process, `--runs` timed calls each after one warm call each;
then each runs `--runs` times back to back, and then the two C entries
alternate on output arrays that are allocated once.

  python tools/parties_measure.py [--out profiles/parties/reconcile_vs_decode_c2.json]

Both entries stage through the same per-device buffers and stream, decode with
the same kernel and copy the same outputs back; reconcile sends n + m + 8
bytes per frame to the device and writes the palette codes there, decode
sends 8 n + m and runs the palettize pass over the LLRs."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "parties", "reconcile_vs_decode_c2.json"))
    args = ap.parse_args()

    import qkd_ldpc_v_amd as Q

    H = Q.load_matrix(os.path.join(ROOT, "tests", "golden", "matrices", "c2_n10240_m2201.alist.gz"), Q._lib.MAT_ALIST)
    g = Q.Graph(H)
    par = Q.Params(Q.SPA, 50, True, 100.0)
    alice, bob, q = Q.bsc_frames(H.n, 0.0215, args.frames, seed=1022025)
    lp = Q.log_p(q)
    syn = g.syndrome(alice)  # Alice's entry; checked against numpy below
    assert np.array_equal(syn, H.syndrome(alice))
    llr = np.where(bob != 0, -lp, lp).astype(np.float64)
    lps = np.full(args.frames, lp)

    def timed(fn):
        t0 = time.perf_counter()
        out = fn()
        return time.perf_counter() - t0, out

    arms = {"reconcile": lambda: g.reconcile(par, bob, lps, syn), "decode": lambda: g.decode(par, llr, syn)}
    ref = {k: fn() for k, fn in arms.items()}  # warm: workspaces, staging buffers, code objects
    same = all(np.array_equal(getattr(ref["reconcile"], f), getattr(ref["decode"], f))
               for f in ("bits", "iterations", "synd_ok"))
    times = {k: [] for k in arms}
    for _ in range(args.runs):
        for k, fn in arms.items():
            t, _ = timed(fn)
            times[k].append(t)
    # ... and each arm back to back (a caller that only ever calls one of them)
    blocked = {k: [timed(fn)[0] for _ in range(args.runs)] for k, fn in arms.items()}
    # ... and the C entries themselves on output arrays allocated once: the
    # wrappers above return fresh numpy arrays, so every call of theirs copies
    # into host memory the runtime has not seen before and frees the last call's
    import ctypes

    from qkd_ldpc_v_amd._lib import lib, ptr

    bits = np.empty((args.frames, H.n), np.uint8)
    iters = np.empty(args.frames, np.uint32)
    ok = np.empty(args.frames, np.uint8)
    p = par.c()
    fixed_arms = {
        "reconcile": lambda: lib().qldpc_reconcile_batch(g.handle, None, ctypes.byref(p), args.frames, ptr(bob),
                                                         ptr(lps), ptr(syn), ptr(bits), ptr(iters), ptr(ok), None),
        "decode": lambda: lib().qldpc_decode_batch(g.handle, ctypes.byref(p), args.frames, ptr(llr), ptr(syn),
                                                   ptr(bits), ptr(iters), ptr(ok), None),
    }
    fixed = {k: [] for k in fixed_arms}
    for i in range(args.runs + 1):  # (one warm round)
        for k, fn in fixed_arms.items():
            t, rc = timed(fn)
            assert rc == 0 and np.array_equal(bits, ref["decode"].bits)
            if i:
                fixed[k].append(t)
    n, m, B = H.n, H.m, args.frames
    res = {
        "what": "wall seconds per call, host buffers in and out, alternating in one process",
        "code": "c2_n10240_m2201.alist", "algorithm": "SPA", "max_iterations": 50, "qber": 0.0215, "frames": B,
        "plan": g.plan(0, Q.SPA),
        "reconcile_s": times["reconcile"], "decode_s": times["decode"],
        "reconcile_mean_s": float(np.mean(times["reconcile"])), "decode_mean_s": float(np.mean(times["decode"])),
        "reconcile_back_to_back_s": blocked["reconcile"], "decode_back_to_back_s": blocked["decode"],
        "reconcile_fixed_outputs_s": fixed["reconcile"], "decode_fixed_outputs_s": fixed["decode"],
        "host_to_device_bytes": {"reconcile": B * (n + m + 8), "decode": B * (8 * n + m)},
        "outputs_equal": bool(same),
        "mean_iterations": float(ref["decode"].iterations.mean()),
        "frames_decoded": int(ref["decode"].synd_ok.sum()),
    }
    res["difference_mean_s"] = res["decode_mean_s"] - res["reconcile_mean_s"]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    if not same:
        raise SystemExit("reconcile and decode disagree")


if __name__ == "__main__":
    main()
