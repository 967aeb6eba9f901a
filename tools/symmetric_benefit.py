"""Fixed-order blind rounds against symmetric ones on INTEGRATION §7's fixture
(C1, 60 punctured and 4 shortened positions, 70 frames at QBER 0.016, SPA
capped at 20 iterations, 20 bits per round): frames decoded per round and the
bits disclosed, both computed with the CPU oracle (tests/test_gpu_blind.np_blind,
tests/symmetric_ref.np_symmetric).  Needs no GPU.  Writes
profiles/blind/symmetric_benefit.json."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import qkd_ldpc_v_amd as Q  # noqa: E402
from symmetric_ref import np_symmetric  # noqa: E402
from test_gpu_blind import BATCH, CAP, PUNCT, QBER, SHORT, STEP, c1_oracle, fixture, np_blind, oracle_params  # noqa: E402

MAX_ROUNDS = 10  # symmetric rounds are not bounded by the punctured list: stop the tabulation here


def table(states, disclosed):
    ok = [s[2] for s in states]
    newly = [int(ok[0].sum())] + [int((ok[r] == 1).sum() - (ok[r - 1] == 1).sum()) for r in range(1, len(ok))]
    return {"decoded_in_round": newly, "decoded_total": int(ok[-1].sum()), "lost": int((ok[-1] == 0).sum()),
            "disclosed_bits_total": int(disclosed.sum()),
            "disclosed_bits_of_decoded_frames": int(disclosed[ok[-1] == 1].sum()),
            "disclosed_per_frame_max": int(disclosed.max())}


alg = (Q.SPA, 0.0, 0.0)
_, _, _, _, ext, syn, llr0 = fixture()
f_states, _, _, f_disc, _ = np_blind(*alg, np.arange(PUNCT.size))
s_states, _, _, s_disc, _, _ = np_symmetric(c1_oracle(), oracle_params(*alg), llr0, syn, ext, SHORT, STEP, MAX_ROUNDS)
res = {"code": "C1", "punctured": int(PUNCT.size), "shortened": int(SHORT.size), "frames": BATCH, "qber": QBER,
       "algorithm": "SPA", "max_iterations": CAP, "step": STEP, "symmetric_max_rounds": MAX_ROUNDS,
       "fixed_order": table(f_states, f_disc), "symmetric": table(s_states, s_disc)}
OUT = os.path.join(ROOT, "profiles", "blind")
os.makedirs(OUT, exist_ok=True)
with open(os.path.join(OUT, "symmetric_benefit.json"), "w") as fh:
    json.dump(res, fh, indent=1)
print(json.dumps(res))
