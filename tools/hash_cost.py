"""Cost of the batched Toeplitz hash (qldpc_toeplitz_hash_device) at a C2-shaped
privacy-amplification point, a 64-bit tag of the same batch and a C4-shaped
point, against the cost model of DESIGN.md ("The Toeplitz hash"): out_len x
ceil(key_len / 32) x 3 lane operations per frame, one wave instruction per
cycle on each of 1024 SIMDs at 2.4 GHz.  Needs the GPU.  Writes
profiles/privacy/hash_cost.json."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import qkd_ldpc_v_amd as Q  # noqa: E402
from toeplitz_ref import toeplitz_ref  # noqa: E402

SIMDS, CLOCK_HZ, OPS_PER_WORD = 1024, 2.4e9, 3
POINTS = {"c2_amplify": (10240, 6144, 4096), "c2_tag": (10240, 64, 4096), "c4_amplify": (102400, 40960, 128)}
WARMUP, CALLS = 3, 10


def predicted_ms(key_len, out_len, batch):
    wave_instructions = batch * out_len * ((key_len + 31) // 32) * OPS_PER_WORD / 64
    return wave_instructions / SIMDS / CLOCK_HZ * 1e3


res = {"model": {"ops_per_key_word_per_output": OPS_PER_WORD, "simds": SIMDS, "clock_hz": CLOCK_HZ},
       "warmup": WARMUP, "calls": CALLS, "points": {}}
for name, (key_len, out_len, batch) in POINTS.items():
    g = torch.Generator(device="cuda").manual_seed(key_len + out_len)
    keys = torch.randint(0, 2, (batch, key_len), dtype=torch.uint8, device="cuda", generator=g)
    seed = torch.randint(0, 2, (key_len + out_len - 1,), dtype=torch.uint8, device="cuda", generator=g)
    out = torch.empty((batch, out_len), dtype=torch.uint8, device="cuda")
    for _ in range(WARMUP):
        Q.toeplitz_hash_device(keys, seed, out)
    torch.cuda.synchronize()
    # what is timed is the right answer: three frames' first 64 outputs against numpy
    rows = [0, batch // 2, batch - 1]
    want = toeplitz_ref(keys[rows].cpu().numpy(), seed[:key_len + 63].cpu().numpy(), 64)
    assert np.array_equal(out[rows, :64].cpu().numpy(), want), name
    ms = []
    for _ in range(CALLS):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        Q.toeplitz_hash_device(keys, seed, out)
        t1.record()
        t1.synchronize()
        ms.append(t0.elapsed_time(t1))
    pred = predicted_ms(key_len, out_len, batch)
    res["points"][name] = {"key_len": key_len, "out_len": out_len, "batch": batch, "ms_per_call": ms,
                           "ms_median": float(np.median(ms)), "ms_min_max": [min(ms), max(ms)],
                           "predicted_ms": pred, "measured_over_predicted": float(np.median(ms)) / pred}
    del keys, seed, out
OUT = os.path.join(ROOT, "profiles", "privacy")
os.makedirs(OUT, exist_ok=True)
with open(os.path.join(OUT, "hash_cost.json"), "w") as fh:
    json.dump(res, fh, indent=1)
print(json.dumps(res))
