"""Cost of the block hash (qldpc_toeplitz_hash_block_device) at three points,
against the cost model of DESIGN.md ("The block hash"), which was written
before the first measurement:

  memory: every pass of a transform reads and writes its 4N bytes; per call
          (n_up = ceil((k - 12) / 7) strided passes): the keys' forward
          transform n_up + 1 passes, the seed's n_up and the fused middle pass
          (two reads, one write), the way back n_up; the top strided pass of
          each transform reads nearly a whole table (4N); the table is written
          once (4N), the pack writes 8N and reads the bytes of keys and seed, the
          extraction reads 4 and writes 1 byte per output; at 6.29 TB/s.
  VALU:   3 k N / 2 butterflies of 27 vector instructions each (the strided
          stage's loop as compiled), 64 lanes per instruction, two cycles per
          instruction on each of 1024 SIMDs at 2.4 GHz.  Two cycles is the
          hardware's floor, not a rate this project has seen: a SIMD has 32
          lanes, so a 64-lane instruction issues over two cycles at best.  The
          per-frame hash's loop was measured at 5 ("The Toeplitz
          hash"); the floor keeps the model free of measurements.
  The model is the larger of the two (launch gaps are not in it).

Point (a) times the block entry beside the existing per-frame kernel
(qldpc_toeplitz_hash_device, one row holding the same key), alternating the two
calls.  HIP events, three warm-up calls and ten timed ones per point; every
point verifies 8 sampled outputs against the index formula before it is timed.
Needs the GPU.  Writes profiles/privacy/hash_block_cost.json.

`--trace NAME` runs five untimed calls of one point and writes nothing: the
program for a kernel trace.  profiles/privacy/hash_block_kernel_stats.csv is the
block kernels' rows of the statistics of
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- \
        python tools/hash_block_cost.py --trace b_c2_batch"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import qkd_ldpc_v_amd as Q  # noqa: E402
from toeplitz_block_ref import toeplitz_at  # noqa: E402

SIMDS, CLOCK_HZ, HBM_BYTES_PER_S = 1024, 2.4e9, 6.29e12
VALU_PER_BUTTERFLY, CYCLES_PER_INSTRUCTION = 27, 2
TILE_LOG, PASS_STAGES = 12, 7
# name -> (frames, key_len, out_len, also time the per-frame kernel on the same key)
POINTS = {"a_24_frames": (24, 10240, 147456, True), "b_c2_batch": (4096, 10240, 1 << 24, False),
          "c_2p20": (1024, 1024, 1 << 19, False)}
WARMUP, CALLS = 3, 10
DECODE_STEP_MS, EXTRAPOLATED_PER_FRAME_MS = 18.05, 800.0  # README.md; the per-frame kernel's rate at point (b)


def model(L, r):
    k = max(L + r - 2, 0).bit_length()
    N = 1 << k
    n_up = -(-max(k - TILE_LOG, 0) // PASS_STAGES)
    words = 2 * (n_up + 1) + (2 * n_up + 3) + 2 * n_up + (3 if n_up else 0) + 1 + 2
    bytes_moved = 4 * N * words + (2 * L + r - 1) + 5 * r
    wave_instructions = 3 * k * (N // 2) * VALU_PER_BUTTERFLY / 64
    mem_ms = bytes_moved / HBM_BYTES_PER_S * 1e3
    valu_ms = wave_instructions * CYCLES_PER_INSTRUCTION / SIMDS / CLOCK_HZ * 1e3
    return {"k": k, "strided_passes": n_up, "bytes": bytes_moved, "memory_ms": mem_ms,
            "butterflies": 3 * k * (N // 2), "valu_ms": valu_ms, "predicted_ms": max(mem_ms, valu_ms),
            "bound": "memory" if mem_ms >= valu_ms else "valu"}


def timed(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1)


def summary(ms):
    return {"ms_per_call": ms, "ms_median": float(np.median(ms)), "ms_min_max": [min(ms), max(ms)]}


ap = argparse.ArgumentParser()
ap.add_argument("--trace", choices=sorted(POINTS), help="five untimed calls of this point, nothing written")
args = ap.parse_args()
if args.trace:
    POINTS, WARMUP, CALLS = {args.trace: POINTS[args.trace][:3] + (False,)}, 5, 0

res = {"model": {"valu_per_butterfly": VALU_PER_BUTTERFLY, "cycles_per_instruction": CYCLES_PER_INSTRUCTION,
                 "simds": SIMDS, "clock_hz": CLOCK_HZ, "hbm_bytes_per_s": HBM_BYTES_PER_S},
       "warmup": WARMUP, "calls": CALLS, "points": {}}
for name, (frames, key_len, out_len, per_frame) in POINTS.items():
    L = frames * key_len
    g = torch.Generator(device="cuda").manual_seed(L + out_len)
    keys = torch.randint(0, 256, (frames, key_len), dtype=torch.uint8, device="cuda", generator=g)
    seed = torch.randint(0, 256, (L + out_len - 1,), dtype=torch.uint8, device="cuda", generator=g)
    out = torch.empty(out_len, dtype=torch.uint8, device="cuda")
    ws = torch.empty(Q.toeplitz_block_workspace(L, out_len), dtype=torch.uint8, device="cuda")
    calls = {"block": lambda: Q.toeplitz_hash_block_device(keys, seed, out, workspace=ws)}
    if per_frame:
        row, out_row = keys.reshape(1, L), torch.empty((1, out_len), dtype=torch.uint8, device="cuda")
        calls["per_frame"] = lambda: Q.toeplitz_hash_device(row, seed, out_row)
    for _ in range(WARMUP):
        for fn in calls.values():
            fn()
    torch.cuda.synchronize()
    # what is timed is the right answer: 8 outputs against the index formula
    idx = np.unique(np.concatenate([[0, out_len - 1], np.random.Generator(np.random.PCG64(5)).integers(0, out_len, 6)]))
    want = toeplitz_at(keys.cpu().numpy().reshape(-1), seed.cpu().numpy(), idx)
    assert np.array_equal(out.cpu().numpy()[idx], want), name
    if per_frame:
        assert np.array_equal(out_row.cpu().numpy()[0], out.cpu().numpy()), name  # the two kernels agree everywhere
    if args.trace:
        continue
    ms = {c: [] for c in calls}
    for _ in range(CALLS):  # (the two calls alternate)
        for c, fn in calls.items():
            ms[c].append(timed(fn))
    point = {"frames": frames, "key_len": key_len, "block_len": L, "out_len": out_len, "workspace_bytes": ws.numel(),
             **summary(ms["block"]), **model(L, out_len)}
    point["measured_over_predicted"] = point["ms_median"] / point["predicted_ms"]
    if per_frame:
        point["per_frame_kernel"] = summary(ms["per_frame"])
        point["block_over_per_frame"] = point["ms_median"] / point["per_frame_kernel"]["ms_median"]
    if name == "b_c2_batch":
        point["over_decode_step"] = point["ms_median"] / DECODE_STEP_MS
        point["extrapolated_per_frame_over_block"] = EXTRAPOLATED_PER_FRAME_MS / point["ms_median"]
    res["points"][name] = point
    del keys, seed, out, ws
if args.trace:
    sys.exit(0)
OUT = os.path.join(ROOT, "profiles", "privacy")
os.makedirs(OUT, exist_ok=True)
with open(os.path.join(OUT, "hash_block_cost.json"), "w") as fh:
    json.dump(res, fh, indent=1)
print(json.dumps(res))
