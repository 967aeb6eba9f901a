"""GPU parity over the decoder's own parameters: thresholds and factors.

The rest of the GPU suite decodes with thr = 100 (which no ordinary message
reaches) or with the threshold off, and with one factor pair per algorithm.
The kernels switch on exactly those values: the SPA scan's lim = min(thr, 44)
and t_lim = tanh(lim / 2.), atanh2_clip's compare against thr, SPA's
iteration-0 table, and ms_clip_later (capi.hip fill_args), which lets the
register kernel leave the min-sum message clip out while |factor| <= 1
(NMSA / ANMSA) or offset >= 0 (OMSA / AOMSA).  Here every one of them is
moved.  The bar is the suite's: hard bits, iteration counts, syndromes_match
and posteriors bitwise equal to the CPU oracle's.

Inputs per case (read-only, built once):
  bsc   BSC frames at the case's QBER, |llr| = log_p
  amp   the same error pattern with |llr| = L (AMP_L: 30 for SPA, 60 for
        min-sum): still a two-entry palette (SPA's iteration-0 table runs)
        and messages grow past 44
  soft  |llr| uniform in [0.25, 40] on the same signs (no palette), 1e-4,
        +-0.0 and DBL_MAX in the first five bits of half the frames

No test passes vacuously; after the parity assertions, on the oracle's arrays
alone ("differs" = posterior bits or iteration count of a frame):
  A  bsc, thr <= 5: the oracle differs from its own threshold-off result in at
     least half the frames
  B  amp, thr in 43.5 .. 60: it differs from threshold-off in >= 2 frames
  C  bsc, SPA and OMSA baselines at thr = 5 (at 12 where C_THR says so): >= 2
     frames stop before the iteration cap and >= 2 reach it
  D  every factor point that makes ms_clip_later 1: at some tested threshold
     the oracle differs from its result at the nearest fine point in >= 2
     frames (the factor is observed, not only the threshold)

The inputs were chosen with the oracle alone (seed 1; BATCH frames per case;
the QBERs in QBER_OWN and tests/test_gpu_shapes.py's QBER, L in AMP_L).  The
oracle's counts with them, the fewest over the thresholds and factor points
of each line; exemptions and their reasons stand at EXEMPT_A / EXEMPT_B:

  case (frames)          A        B        C: early/capped, SPA | OMSA          D
  c1 (12)                11       SPA 9, a1/b0 10, b50 4, rest 12
                                           8/4 | 5/7                            12
  degree1_rows (12)      12       SPA 10, rest 12
                                           5/7 at thr 12 | 3/9                  12
  hybrid_dv4_global (8)  8        8        4/4 (QBER 0.014) | 3/5               8
  split_k4 (9)           9        9        6/3 at thr 12 | 6/3                  9
  long_row33 (8)         8        8        4/4 at thr 12 | 2/6                  8
  long_row41 (8)         8        8        4/4 at thr 12 | 3/5                  8
  c1_fpl, c1_v1 (8)      7        SPA 7, rest 8
                                           5/3 | 4/4                            8
  c1_vng0 (8)            7        8        - | 4/4                              8
  c3_vng0 (8)            8        8        - | 2/6 (QBER 0.017)                 8
  c1 soft, thr 1 and 12: SPA 6 of 12 frames differ from threshold-off, the rest 12
  c1 caps at thr 1: amp cap 1 and bsc / amp cap 2 differ in 12 of 12 (SPA, bsc, cap 1: 0)
"""
import contextlib
import functools
import math
import sys

import numpy as np
import pytest

import qkd_ldpc_v_amd as Q
import shape_codes as S
import test_gpu_parity as P
import test_gpu_shapes as G
from conftest import bits_equal_nan, diag_env, load_fixture
from oracle.pyoracle import Oracle
from test_gpu_parity import ALGS, frames, math_inputs
from test_shape_plans import matrix as shape_matrix

pytestmark = pytest.mark.gpu

DBL_MAX = sys.float_info.max
INF, NAN = math.inf, math.nan
CAP = 50
SEED = 1
C1, C3 = "c1_n1024_m220.alist", "c3_n10240_m1801.alist"
NAMES = {Q.SPA: "SPA", Q.SPA_LIN: "SPA_LIN", Q.NMSA: "NMSA", Q.OMSA: "OMSA", Q.ANMSA: "ANMSA", Q.AOMSA: "AOMSA"}

THRS = (1e-3, 1.0, 5.0, 12.0, 37.0, 37.5, 43.5, 44.0, 44.5, 60.0, 1e300, INF)
THRS_SOFT = (1.0, 12.0, 43.5, 60.0)
THRS_REDUCED = (1.0, 5.0, 43.5, 60.0)
BITING = (43.5, 44.0, 44.5, 60.0)       # condition B


def LOW(thr):                           # condition A
    return thr <= 5.0


# factor points: id -> (algorithm, primary, secondary); the first of each algorithm is ALGS's
POINTS = {NAMES[a]: (a, p, s) for a, p, s in ALGS}
POINTS.update({
    "NMSA_a1": (Q.NMSA, 1.0, 0.0),                                  # boundary, fine
    "NMSA_a1next": (Q.NMSA, math.nextafter(1.0, 2.0), 0.0),          # not fine by one ulp
    "NMSA_a1.25": (Q.NMSA, 1.25, 0.0),                              # not fine
    "NMSA_a-0.5": (Q.NMSA, -0.5, 0.0),                              # fine, sign-flipping
    "NMSA_a-1.25": (Q.NMSA, -1.25, 0.0),                            # not fine, sign-flipping
    "NMSA_a0": (Q.NMSA, 0.0, 0.0),                                  # every message +-0
    "NMSA_nan": (Q.NMSA, NAN, 0.0),                                 # every message NaN
    "OMSA_b0": (Q.OMSA, 0.0, 0.0),                                  # boundary, fine
    "OMSA_b-0.4": (Q.OMSA, -0.4, 0.0),                              # not fine: messages exceed sel
    "OMSA_b50": (Q.OMSA, 50.0, 0.0),                                # every message 0 (but a one-edge row's)
    "OMSA_nan": (Q.OMSA, NAN, 0.0),
    "ANMSA_nu1.3": (Q.ANMSA, 0.8, 1.3),                             # secondary only not fine
    "ANMSA_a1.2": (Q.ANMSA, 1.2, 0.5),                              # primary only
    "AOMSA_s-0.3": (Q.AOMSA, 0.55, -0.3),
    "AOMSA_b-0.2": (Q.AOMSA, -0.2, 1.2),
})
BASELINES = [NAMES[a] for a, _, _ in ALGS]
NOT_FINE_ONE_EACH = ["NMSA_a1.25", "OMSA_b-0.4", "ANMSA_nu1.3", "AOMSA_b-0.2"]
REDUCED = BASELINES + NOT_FINE_ONE_EACH
MINSUM_REDUCED = [p for p in REDUCED if POINTS[p][0] >= Q.NMSA]


def fine(point):
    """capi.hip fill_args: ms_clip_later == 0."""
    alg, prim, sec = POINTS[point]
    ok = (lambda x: abs(x) <= 1.0) if alg in (Q.NMSA, Q.ANMSA) else (lambda x: x >= 0.0)
    return alg < Q.NMSA or (ok(prim) and (alg in (Q.NMSA, Q.OMSA) or ok(sec)))


def nearest_fine(point):
    """-> (alg, primary, secondary) with each not-fine factor moved to the
    nearest fine value (+-1.0 / 0.0; NaN to 1.0 / 0.0)."""
    alg, prim, sec = POINTS[point]
    if alg in (Q.NMSA, Q.ANMSA):
        near = lambda x: x if abs(x) <= 1.0 else (math.copysign(1.0, x) if x == x else 1.0)
    else:
        near = lambda x: x if x >= 0.0 else 0.0
    return alg, near(prim), near(sec) if alg >= Q.ANMSA else sec


# ---- cases ------------------------------------------------------------------------------------------
# case -> frames.  c1* / c3* are the committed fixtures (c1 1024 x 220, c3 10240 x 1801), the others
# tests/shape_codes.py's; *_vng0 decodes under QLDPC_VNG=0 (min-sum through the VN phases).
BATCH = {"c1": 12, "degree1_rows": 12, "hybrid_dv4_global": 8, "split_k4": 9, "long_row33": 8, "long_row41": 8,
         "c1_fpl": 8, "c1_vng0": 8, "c3_vng0": 8, "c1_v1": 8}
FULL_CASES = ["c1", "degree1_rows"]
REDUCED_CASES = ["hybrid_dv4_global", "split_k4", "long_row33", "long_row41", "c1_fpl", "c1_vng0", "c3_vng0", "c1_v1"]

# QBER of the bsc / amp frames: case -> (QBER, {point or algorithm: its own}).  A case that is not
# here takes tests/test_gpu_shapes.py's; the ones here have none there (c1, c3) or need another under
# a low threshold.
QBER_OWN = {
    "c1": (0.02, {"NMSA_a1": 0.0125, "NMSA_a1next": 0.0125, "OMSA_b0": 0.0125, "AOMSA_s-0.3": 0.015}),
    "c3": (0.017, {}),
    "hybrid_dv4_global": (0.022, {"SPA": 0.014}),
}
# |llr| of the amp frames: by algorithm, then the points with their own.  SPA needs L < 44 (beyond it
# tanh(L / 2.) is 1 and every message +-inf before the clip); min-sum messages start at L.
AMP_L = {Q.SPA: 30.0, Q.SPA_LIN: 30.0, Q.NMSA: 60.0, Q.OMSA: 60.0, Q.ANMSA: 60.0, Q.AOMSA: 60.0}
AMP_L_OWN = {("c1", "NMSA_a-0.5"): 100.0}
# Condition C's threshold where SPA reaches no frame's syndrome under thr = 5 at any QBER tried
# (0.004 .. 0.02): 12.0, which the tests of those cases then decode as well.
C_THR = {("degree1_rows", "SPA"): 12.0, ("split_k4", "SPA"): 12.0, ("long_row33", "SPA"): 12.0,
         ("long_row41", "SPA"): 12.0}
# Points that cannot meet condition A or B, by case ("*": every case) -> {point: thresholds, None = all}:
#   NMSA_a0       every message is +-0 and the posterior the channel LLR, clipped or not
#   NMSA_nan, OMSA_nan   every message and posterior is NaN, which the clip passes
#   OMSA_b50      every message is 0 on c1 (min - 50 < 0); degree1_rows' one-edge rows send DBL_MAX - 50
#   NMSA_a-0.5    c1, bsc, thr = 5: 0 of 12 at every QBER from 0.01 to 0.04 (sign-flipping messages of
#                 half the minimum stay below 5); thr <= 1 and the amp frames hold
#   SPA_LIN       B: its messages are at most 2 * atanh_lin(1) = 10 and tanh_lin(x / 2.) is 1 from
#                 |x| = 16 on, so no clip at 43.5 or above is visible at any L
EXEMPT_A = {"*": {"NMSA_a0": None, "NMSA_nan": None, "OMSA_nan": None},
            "c1": {"OMSA_b50": None, "NMSA_a-0.5": (5.0,)}}
EXEMPT_B = {"*": {"SPA_LIN": None, "NMSA_a0": None, "NMSA_nan": None, "OMSA_nan": None}}


def exempt(table, case, point, thr):
    for key in ("*", base(case)):
        if point in table.get(key, {}):
            thrs = table[key][point]
            if thrs is None or thr in thrs:
                return True
    return False


_graphs, _oracles = {}, {}


def base(case):
    return case.split("_")[0] if case.startswith(("c1", "c3")) else case


def H_of(case):
    b = base(case)
    return load_fixture({"c1": C1, "c3": C3}[b]) if b in ("c1", "c3") else shape_matrix(case)


def graph(case):
    if case in ("c1", "c1_vng0"):
        return P.graph(C1)
    if case == "c3_vng0":
        return P.graph(C3)
    if case == "c1_v1":
        return P.graph(C1, "v1")
    if case == "c1_fpl":
        if case not in _graphs:
            _graphs[case] = Q.Graph(H_of(case), layout="frame_per_lane")
        return _graphs[case]
    return G.graph(case)


def oracle(case):
    b = base(case)
    if b not in _oracles:
        _oracles[b] = Oracle(H_of(case))
    return _oracles[b]


def decode_env(case):
    return diag_env(QLDPC_VNG="0") if case.endswith("_vng0") else contextlib.nullcontext()


def qber(case, point):
    """A point's own QBER, else its algorithm's, else the case's."""
    q, own = QBER_OWN[base(case)] if base(case) in QBER_OWN else G.QBER[case]
    return own.get(point, own.get(POINTS[point][0], q))


def amp_l(case, point):
    return AMP_L_OWN.get((base(case), point), AMP_L[POINTS[point][0]])


def thresholds(case, point, thrs):
    """thrs, and condition C's own threshold for this case and point where it has one."""
    own = C_THR.get((base(case), point))
    return thrs if own is None or own in thrs else tuple(sorted(thrs + (own,)))


@functools.lru_cache(maxsize=None)
def inputs(case, kind, point):
    """-> (llr, syndromes) of a case's frames for a factor point; shared and read-only."""
    H = H_of(case)
    _, b, llr, synd = frames(H, qber(case, point), BATCH[case], SEED)
    sign = np.where(b != 0, -1.0, 1.0)
    if kind == "amp":
        llr = sign * amp_l(case, point)
    elif kind == "soft":
        llr = sign * np.random.default_rng(5).uniform(0.25, 40.0, sign.shape)
        llr[::2, :5] = [1e-4, -1e-4, 0.0, -0.0, DBL_MAX]
    else:
        assert kind == "bsc"
    llr.setflags(write=False)
    synd.setflags(write=False)
    return llr, synd


@functools.lru_cache(maxsize=None)
def oracle_result(case, kind, point, thr, max_it=CAP):
    """(bits, iterations, ok, posterior) of the oracle; thr None = threshold
    off; point an id of POINTS.  Computed once, shared, read-only."""
    alg, prim, sec = POINTS[point]
    llr, synd = inputs(case, kind, point)
    O = oracle(case)
    on = thr is not None
    ref = O.decode_batch(O.params(alg, max_it, on, thr if on else 100.0, prim, sec), llr, synd, threads=16,
                         posterior=True)
    for x in ref:
        x.setflags(write=False)
    return ref


def oracle_at(case, kind, point, alg, prim, sec, thr, max_it=CAP):
    """The same on a point's frames at other factors (condition D's fine neighbours)."""
    llr, synd = inputs(case, kind, point)
    O = oracle(case)
    return O.decode_batch(O.params(alg, max_it, True, thr, prim, sec), llr, synd, threads=16, posterior=True)


def differing(r1, r2):
    """Frames whose posterior bits or iteration count differ between two results."""
    return sum(1 for f in range(r1[1].size) if r1[1][f] != r2[1][f] or not bits_equal_nan(r1[3][f], r2[3][f]))


def assert_parity(case, point, kind, thr, max_it=CAP):
    alg, prim, sec = POINTS[point]
    llr, synd = inputs(case, kind, point)
    on = thr is not None
    with decode_env(case):
        out = graph(case).decode(Q.Params(alg, max_it, on, thr if on else 100.0, prim, sec), llr, synd, posterior=True)
    ob, oi, ok, op = ref = oracle_result(case, kind, point, thr, max_it)
    bad = [f for f in range(llr.shape[0])
           if not (np.array_equal(out.bits[f], ob[f]) and out.iterations[f] == oi[f] and out.synd_ok[f] == ok[f]
                   and bits_equal_nan(out.posterior[f], op[f]))]
    assert not bad, (f"{case} {point} {kind} thr={thr} cap={max_it}: {len(bad)}/{llr.shape[0]} frames differ; first "
                     f"{bad[0]}: gpu it={out.iterations[bad[0]]} ok={out.synd_ok[bad[0]]} / oracle it={oi[bad[0]]} "
                     f"ok={ok[bad[0]]}; bit diffs={int((out.bits[bad[0]] != ob[bad[0]]).sum())}; posterior diffs="
                     f"{int((~((out.posterior[bad[0]] == op[bad[0]]) | (np.isnan(out.posterior[bad[0]]) & np.isnan(op[bad[0]])))).sum())}")
    return ref


# ---- the conditions, on the oracle's arrays -------------------------------------------------------
def count_a(case, point, thr, max_it=CAP, kind="bsc"):
    return differing(oracle_result(case, kind, point, thr, max_it), oracle_result(case, kind, point, None, max_it))


def count_b(case, point, thr):
    return differing(oracle_result(case, "amp", point, thr), oracle_result(case, "amp", point, None))


def spread_c(case, point, thr=None):
    thr = C_THR.get((base(case), point), 5.0) if thr is None else thr
    oi = oracle_result(case, "bsc", point, thr)[1]
    return int((oi < CAP).sum()), int((oi == CAP).sum())


def count_d(case, point, thrs, kinds=("bsc", "amp")):
    """The most frames in which a not-fine point differs from its nearest fine point."""
    alg, prim, sec = nearest_fine(point)
    return max(differing(oracle_result(case, kind, point, thr), oracle_at(case, kind, point, alg, prim, sec, thr))
               for kind in kinds for thr in thrs)


def assert_conditions(case, point, thrs):
    alg = POINTS[point][0]
    n = BATCH[case]
    for thr in thrs:
        if LOW(thr) and not exempt(EXEMPT_A, case, point, thr):
            assert 2 * count_a(case, point, thr) >= n, f"A: {case} {point} thr={thr}: {count_a(case, point, thr)}/{n}"
        if thr in BITING and not exempt(EXEMPT_B, case, point, thr):
            assert count_b(case, point, thr) >= 2, f"B: {case} {point} thr={thr}: {count_b(case, point, thr)}/{n}"
    if point in ("SPA", "OMSA"):
        assert C_THR.get((base(case), point), 5.0) in thrs
        early, capped = spread_c(case, point)
        assert early >= 2 and capped >= 2, f"C: {case} {point}: {early} early, {capped} at the cap"
    if not fine(point):
        assert count_d(case, point, thrs) >= 2, f"D: {case} {point}"


def assert_case_plan(case, alg):
    """The plan each case was chosen for, after the bits."""
    g = graph(case)
    if case in S.PLANS:
        S.assert_plan(g, case, alg)
    elif case == "c1_fpl":
        assert g.plan(0, alg)["variant"] == "fpl", g.plan(0, alg)
    else:
        assert g.plan(0, alg)["variant"] == ("reg_lds" if case == "c1_v1" else "v2"), (case, g.plan(0, alg))


# ---- the full cross on the two smallest register cases --------------------------------------------
@pytest.mark.parametrize("point", list(POINTS))
@pytest.mark.parametrize("case", FULL_CASES)
def test_thresholds_by_factors_full_cross(gpu_available, case, point):
    """Every threshold point on bsc and amp frames.  degree1_rows' one-edge rows
    keep min2 = DBL_MAX, the only way past the register kernel's elided clip
    while the factors are fine (the per-scan `big` flag)."""
    for kind in ("bsc", "amp"):
        for thr in THRS:
            assert_parity(case, point, kind, thr)
    assert_conditions(case, point, THRS)
    assert_case_plan(case, POINTS[point][0])


@pytest.mark.parametrize("point", BASELINES)
def test_c1_soft_frames(gpu_available, point):
    """No palette: the general iteration 0 and llr[] from HBM, specials in half the frames."""
    for thr in THRS_SOFT:
        assert_parity("c1", point, "soft", thr)
    off = oracle_result("c1", "soft", point, None)
    assert all(differing(oracle_result("c1", "soft", point, thr), off) >= 2 for thr in (1.0, 12.0)), point
    assert_case_plan("c1", POINTS[point][0])


@pytest.mark.parametrize("point", BASELINES)
def test_c1_iteration_caps_under_a_low_threshold(gpu_available, point):
    """thr = 1.0 is below the channel magnitude: iteration 0 reads the
    unclipped channel LLR and clips what it sends, iteration 1 is the first to
    read clipped messages.  Caps 1 and 2 are the exit edges of both."""
    for max_it in (1, 2):
        for kind in ("bsc", "amp", "soft"):
            assert_parity("c1", point, kind, 1.0, max_it)
    # the clip is seen at both caps: on the amp frames from the first messages on, on the bsc frames
    # from iteration 1 on (SPA's first messages, 2 atanh of a product of 14 tanh(log_p / 2.), are below 1)
    assert 2 * count_a("c1", point, 1.0, 1, "amp") >= BATCH["c1"], point
    assert 2 * min(count_a("c1", point, 1.0, 2, kind) for kind in ("bsc", "amp")) >= BATCH["c1"], point
    assert_case_plan("c1", POINTS[point][0])


# ---- the other kernel families with message or clip code of their own --------------------------
def _reduced_params():
    for case in REDUCED_CASES:
        for point in (MINSUM_REDUCED if case.endswith("_vng0") else REDUCED):
            yield case, point


@pytest.mark.parametrize("case,point", list(_reduced_params()))
def test_thresholds_by_factors_other_families(gpu_available, case, point):
    """hybrid_dv4_global: RGLB rows and the bit gather's ms_message; split_k4:
    SPLIT forces the clip and defers the exit; long_row33 / long_row41 and
    c1_v1: the first-generation kernels (reg_lds, glb_lds); c1_fpl: the
    frame-per-lane layout; *_vng0: min-sum through the VN phases."""
    thrs = thresholds(case, point, THRS_REDUCED)
    for kind in ("bsc", "amp"):
        for thr in thrs:
            assert_parity(case, point, kind, thr)
    assert_conditions(case, point, thrs)
    assert_case_plan(case, POINTS[point][0])


# ---- the clipped forms themselves at other thresholds ----------------------------------------------
C_TOP = 2.0 * math.atanh(1.0 - 2.0**-53)


def _neighbours(v):
    return [math.nextafter(v, -INF), v, math.nextafter(v, INF)]


@functools.lru_cache(maxsize=None)
def _clip_inputs():
    """test_device_exact_math_bitwise's inputs, then +-thr, +-lim and +-c_top
    with both neighbours for every threshold, and the products p whose
    2 atanh(p) straddles the threshold (p = tanh(thr / 2.) +- 4 ulp)."""
    extra = []
    for thr in MATH_THRS:
        for v in {thr, min(thr, 44.0), C_TOP}:
            if v < INF:
                extra += _neighbours(v)
        p = math.tanh(thr / 2.0)
        for _ in range(4):
            p = math.nextafter(p, INF)
        for _ in range(9):
            extra.append(p)
            p = math.nextafter(p, -INF)
    extra = np.array(extra)
    xs = np.concatenate([math_inputs(), extra, -extra])
    xs.setflags(write=False)

    def atanh2(x):
        try:
            return 2.0 * math.atanh(x)
        except ValueError:  # C atanh: +-1 -> +-inf, beyond -> NaN
            return math.copysign(INF, x) if abs(x) == 1 else NAN
    tanh_half = np.array([math.tanh(float(x) / 2.0) for x in xs])
    atanh_two = np.array([atanh2(float(x)) for x in xs])
    return xs, tanh_half, atanh_two


MATH_THRS = (1e-3, 1.0, 12.0, 37.0, 37.5, 43.5, 44.0, 60.0, INF)


@pytest.mark.parametrize("thr", MATH_THRS)
def test_device_clipped_forms_bitwise(gpu_available, thr):
    """fn 8 = tanh_half_clip_t(x, lim, t_lim) against math.tanh(clip(x, thr) / 2.)
    and fn 9 = atanh2_clip(x, thr, c_top) against clip(2. * math.atanh(x), thr),
    with lim, t_lim and c_top from the host code of a decode launch."""
    import torch

    xs, tanh_half, atanh_two = _clip_inputs()
    over = np.abs(xs) > thr  # the reference's threshold_matrix: |v| > thr -> +-thr, NaN passes
    want8 = np.where(over, np.copysign(math.tanh(thr / 2.0), xs), tanh_half)
    want9 = np.where(np.abs(atanh_two) > thr, np.copysign(thr, atanh_two), atanh_two)
    d_in = torch.tensor(xs, device="cuda")  # (a copy: xs is shared and read-only)
    d_out = torch.empty_like(d_in)
    for fn, want in ((8, want8), (9, want9)):
        Q._lib.check(Q.lib().qldpc_selftest_math_thr_device(fn, thr, xs.size, d_in.data_ptr(), d_out.data_ptr(), None),
                     "selftest")
        torch.cuda.synchronize()
        got = d_out.cpu().numpy()
        bad = np.nonzero(~((got.view(np.uint64) == want.view(np.uint64)) | (np.isnan(got) & np.isnan(want))))[0]
        assert bad.size == 0, (f"fn {fn} thr={thr}: {bad.size} diffs; first x={xs[bad[0]]!r} got={got[bad[0]]!r} "
                               f"want={want[bad[0]]!r}")
    # the clip was reached from both sides: inputs clipped and inputs just short of it
    if thr < INF:
        finite = atanh_two[np.isfinite(atanh_two)]
        assert over.any() and (~over).any() and (thr > C_TOP or ((np.abs(finite) > thr).any() and
                                                                 (np.abs(finite) <= thr).any()))
