#!/usr/bin/env python3
"""Cost of the per-iteration trace on a frame-per-lane graph:
C2 SPA, cap 50, the decode's kernel-event milliseconds (set_kernel_timing)
without and with the trace, three runs each, the two arms alternated in one
process: 4096 frames against counts only, 64 frames against counts plus
posteriors.  One JSON line per run (profiles/trace/trace_cost_c2_spa.jsonl).

  python tools/trace_cost.py
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import qkd_ldpc_v_amd as Q  # noqa: E402
from conftest import load_fixture  # noqa: E402


def run(g, H, p, batch, mode):
    dev = torch.device("cuda:0")
    a, b, q = Q.bsc_frames(H.n, 0.0215, batch, seed=5)
    lp = Q.log_p(q)
    tl = torch.from_numpy(np.where(b != 0, -lp, lp).astype(np.float64)).to(dev)
    ts = torch.from_numpy(H.syndrome(a)).to(dev)
    bits = torch.empty((batch, H.n), dtype=torch.uint8, device=dev)
    it = torch.empty(batch, dtype=torch.int32, device=dev)
    ok = torch.empty(batch, dtype=torch.uint8, device=dev)
    unsat = torch.empty((batch, 50), dtype=torch.int32, device=dev)
    tpost = torch.empty((batch, 50, H.n), dtype=torch.float64, device=dev) if mode == "counts+posteriors" else None

    def once(traced):
        if traced:
            g.decode_trace_device(p, tl, ts, bits, it, ok, None, unsat, tpost)
        else:
            g.decode_device(p, tl, ts, bits, it, ok, None)
        return g.last_decode_kernel_ms()

    once(False), once(True)  # warm: workspaces
    for r in range(3):
        for traced in (False, True):
            ms = once(traced)
            print(json.dumps({"workload": "c2 SPA cap 50, frame_per_lane", "frames": batch, "run": r,
                              "trace": mode if traced else "none", "kernel_ms": round(ms, 3),
                              "mean_iterations": float(it.float().mean())}), flush=True)


def main():
    H = load_fixture("c2_n10240_m2201.alist")
    g = Q.Graph(H, layout="frame_per_lane")
    g.set_kernel_timing(True)
    p = Q.Params(Q.SPA, 50, True, 100.0)
    run(g, H, p, 4096, "counts")
    run(g, H, p, 64, "counts+posteriors")


if __name__ == "__main__":
    main()
