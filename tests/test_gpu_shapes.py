"""GPU parity on the kernel shapes and row structures no committed matrix plans.

Every graph is generated (tests/shape_codes.py) or a committed fixture under a
forced wave count; tests/test_shape_plans.py pins the plan of each on the CPU
and every test here asserts it again, after the bits, on the device graph.
The bar is tests/test_gpu_parity.py's: hard bits, iteration counts,
syndromes_match and posterior LLRs bitwise equal to the CPU oracle's.

Inputs are not degenerate: wherever a test decodes BSC frames with the default
iteration cap, the oracle's own SPA and OMSA results hold at least two frames
that stop before the cap and two that reach it (assert_spread, on the oracle's
arrays, after the parity assertion).  The QBERs were chosen with the oracle
alone, 12 / 9 / 8 frames of seed 1; where SPA and OMSA cannot share one, each
has its own (QBER below: a default per case, then per algorithm).
"""
import contextlib
import sys

import numpy as np
import pytest

import qkd_ldpc_v_amd as Q
import shape_codes as S
from conftest import bits_equal_nan, diag_env
from oracle.pyoracle import Oracle
from test_gpu_parity import ALGS, frames
from test_shape_plans import matrix

pytestmark = pytest.mark.gpu

DBL_MAX = sys.float_info.max
CAP = 50
SPA, OMSA, AOMSA = ALGS[0], ALGS[3], ALGS[5]
MINSUM = (Q.NMSA, Q.OMSA, Q.ANMSA, Q.AOMSA)

# case -> (QBER, {algorithm: its own QBER}); early / capped frames of the oracle in the comments
QBER = {
    "reg44": (0.022, {}),                                          # SPA 10/2, OMSA 6/6 of 12
    "reg44_full": (0.0235, {Q.OMSA: 0.022}),                        # SPA 8/4, OMSA 7/5 (AOMSA 4/8)
    "c2_w12": (0.0215, {Q.SPA: 0.0233, Q.OMSA: 0.022}),             # SPA 3/5, OMSA 5/3 of 8 (0.0215: 8/0, 7/1)
    "c1_w2": (0.02, {}), "c1_w3": (0.02, {}),                      # SPA 9/3, OMSA 5/7
    "hybrid_dv4_lds": (0.022, {Q.SPA: 0.0225}),                     # SPA 8/4, OMSA 4/8 (SPA at 0.022: 11/1)
    "hybrid_dv4_global": (0.022, {Q.SPA: 0.0225}),                  # SPA 9/3, OMSA 2/10 (SPA at 0.022: 11/1)
    "split_k4": (0.018, {Q.SPA: 0.019}),                            # SPA 6/3, OMSA 7/2 of 9 (SPA at 0.018: 9/0)
    "split_k2_w8": (0.08, {Q.SPA: 0.082, Q.OMSA: 0.0765}),          # SPA 4/4, OMSA 5/3 of 8 (AOMSA 5/3)
    "split_k2_w16": (0.0195, {Q.SPA: 0.020, Q.OMSA: 0.019}),        # SPA 4/4, OMSA 4/4 of 8 (AOMSA 4/4)
    "degree1_rows": (0.012, {}),                                    # SPA 5/7, OMSA 5/7
    "short_rows": (0.03, {Q.SPA: 0.008, Q.OMSA: 0.10}),             # SPA 7/5, OMSA 6/6
    "row_starts_32": (0.012, {Q.OMSA: 0.2}),                        # SPA 8/4, OMSA 3/9
    "long_row32": (0.008, {}),                                      # SPA 7/5, OMSA 5/7
    "long_row33": (0.008, {}), "long_row40": (0.008, {}), "long_row41": (0.008, {}),  # SPA 7/5, OMSA 5/7 (41: 6/6)
    "degree510_bit": (0.01, {}),                                    # SPA 2/10
    "empty_row_first": (0.010, {}), "empty_row_last": (0.010, {}),  # 8/4 before the empty row's bit is set
    "reg44_isolated": (0.024, {Q.OMSA: 0.0225}),                    # SPA 6/6, OMSA 8/4
    "split_k4_isolated": (0.020, {}),                               # SPA 5/4, OMSA 2/7 of 9
}
_graphs, _oracles = {}, {}


def qber(case, alg):
    q, own = QBER[case]
    return own.get(alg, q)


def graph(case):
    """Device graph of a case, built once per module (QLDPC_V2_WAVES is read
    when the graph is created, under the diagnostic switch)."""
    if case not in _graphs:
        with diag_env(**S.KNOBS[case]) if case in S.KNOBS else contextlib.nullcontext():
            _graphs[case] = Q.Graph(matrix(case))
    return _graphs[case]


def oracle(case):
    if case not in _oracles:
        _oracles[case] = Oracle(matrix(case))
    return _oracles[case]


def assert_parity(case, alg, prim, sec, llr, synd, max_it=CAP, thr_on=True):
    """Decode (llr, synd) on the case's graph: bits, iterations, syndromes_match
    and posteriors bitwise equal to the oracle's.  -> (out, (bits, iterations,
    ok, posterior) of the oracle)."""
    g, O = graph(case), oracle(case)
    out = g.decode(Q.Params(alg, max_it, thr_on, 100.0, prim, sec), llr, synd, posterior=True)
    ref = O.decode_batch(O.params(alg, max_it, thr_on, 100.0, prim, sec), llr, synd, threads=16, posterior=True)
    ob, oi, ok, op = ref
    bad = [f for f in range(llr.shape[0])
           if not (np.array_equal(out.bits[f], ob[f]) and out.iterations[f] == oi[f] and out.synd_ok[f] == ok[f]
                   and bits_equal_nan(out.posterior[f], op[f]))]
    assert not bad, (f"{case} alg={alg} cap={max_it} thr={thr_on}: {len(bad)}/{llr.shape[0]} frames differ; first "
                     f"{bad[0]}: gpu it={out.iterations[bad[0]]} ok={out.synd_ok[bad[0]]} / oracle it={oi[bad[0]]} "
                     f"ok={ok[bad[0]]}; bit diffs={int((out.bits[bad[0]] != ob[bad[0]]).sum())}")
    return out, (ob, oi, ok, op)


def assert_spread(alg, oi, max_it=CAP):
    """SPA and OMSA: the oracle's own result is not degenerate."""
    if alg in (Q.SPA, Q.OMSA):
        early, capped = int((oi < max_it).sum()), int((oi == max_it).sum())
        assert early >= 2 and capped >= 2, f"degenerate input for alg={alg}: {early} early, {capped} at the cap"


def bsc_parity(case, alg, prim, sec, batch, seed=1, spread=True, **kw):
    """BSC frames at the case's QBER for this algorithm."""
    q = qber(case, alg)
    _, _, llr, synd = frames(matrix(case), q, batch, seed)
    out, ref = assert_parity(case, alg, prim, sec, llr, synd, **kw)
    if spread and kw.get("max_it", CAP) == CAP:
        assert_spread(alg, ref[1])
    return out, ref


# ---- 44-slot register shape (pick_v2<V2_R_SMALL, 0>) ---------------------------------------------
@pytest.mark.parametrize("alg,prim,sec", ALGS)
def test_reg44_all_algorithms(gpu_available, alg, prim, sec):
    """C2's size with other edges: 44 slots, 41 used.  Min-sum takes the
    VN-phase path here by default (the bit gather needs the 40-slot shape)."""
    bsc_parity("reg44", alg, prim, sec, 12)
    S.assert_plan(graph("reg44"), "reg44", alg)


@pytest.mark.parametrize("alg,prim,sec", [SPA, OMSA, AOMSA])
def test_reg44_full_lanes(gpu_available, alg, prim, sec):
    """Every slot of the fullest lanes holds an edge (epl 44)."""
    bsc_parity("reg44_full", alg, prim, sec, 12)
    S.assert_plan(graph("reg44_full"), "reg44_full", alg)


@pytest.mark.parametrize("alg,prim,sec", ALGS)
def test_reg44_iteration_caps_and_threshold_off(gpu_available, alg, prim, sec):
    for max_it in (1, 2, 3):
        bsc_parity("reg44", alg, prim, sec, 8, seed=2, max_it=max_it)
    bsc_parity("reg44", alg, prim, sec, 8, seed=3, thr_on=False, spread=False)
    S.assert_plan(graph("reg44"), "reg44", alg)


@pytest.mark.parametrize("alg,prim,sec", ALGS)
def test_reg44_soft_and_special_llrs(gpu_available, alg, prim, sec):
    """More than 4 distinct LLRs per frame (no palette) with 1e-4, +-0.0 and
    DBL_MAX in half the frames; NaN and +-inf channel LLRs in others."""
    H = matrix("reg44")
    _, _, llr, s = frames(H, 0.021, 8, 4)
    llr = llr * np.random.default_rng(5).uniform(0.6, 1.4, llr.shape)
    llr[::2, :5] = [1e-4, -1e-4, 0.0, -0.0, DBL_MAX]
    assert_parity("reg44", alg, prim, sec, llr, s)
    _, _, llr, s = frames(H, 0.021, 8, 6)
    llr[0, 5] = np.nan
    llr[1, [7, 9]] = [np.inf, -np.inf]
    llr[2, [11, 12, 13]] = [np.nan, np.inf, -np.inf]
    assert_parity("reg44", alg, prim, sec, llr, s)
    S.assert_plan(graph("reg44"), "reg44", alg)


@pytest.mark.parametrize("alg,prim,sec", ALGS)
def test_reg44_rate_adapted_palette(gpu_available, alg, prim, sec):
    """300 punctured (1e-4) and 200 shortened (DBL_MAX) positions: a full
    four-entry palette, threshold on and off."""
    H = matrix("reg44")
    a, b, _, _ = frames(H, 0.02, 8, 7)
    pos = np.random.default_rng(8).permutation(H.n)
    punct, short = pos[:300], pos[300:500]
    a[:, short] = 0
    b[:, short] = 0
    lp = Q.log_p(0.02)
    llr = np.where(b != 0, -lp, lp)
    llr[:, punct] = 1e-4
    llr[:, short] = DBL_MAX
    s = H.syndrome(a)
    for thr_on in (True, False):
        assert_parity("reg44", alg, prim, sec, llr, s, thr_on=thr_on)
    S.assert_plan(graph("reg44"), "reg44", alg)


# ---- 56-slot register shape (pick_v2<V2_R_MID, 0>) and forced wave counts ------------------------
@pytest.mark.parametrize("alg,prim,sec", ALGS)
def test_c2_56_slot_shape_all_algorithms(gpu_available, alg, prim, sec):
    """No graph found plans 56 slots on 768 lanes on its own: c2 under
    QLDPC_V2_WAVES=12.  Iteration caps 1-3 for SPA and OMSA."""
    bsc_parity("c2_w12", alg, prim, sec, 8)
    if alg in (Q.SPA, Q.OMSA):
        for max_it in (1, 2, 3):
            bsc_parity("c2_w12", alg, prim, sec, 8, seed=2, max_it=max_it)
    S.assert_plan(graph("c2_w12"), "c2_w12", alg)


@pytest.mark.parametrize("alg,prim,sec", [SPA, OMSA])
@pytest.mark.parametrize("case", ["c1_w2", "c1_w3"])
def test_c1_forced_wave_counts(gpu_available, case, alg, prim, sec):
    """c1 on 2 waves (every slot of the 40 used) and on 3, an odd count."""
    bsc_parity(case, alg, prim, sec, 12)
    S.assert_plan(graph(case), case, alg)


# ---- hybrid shape with dv_max <= 4: no high-degree stage -----------------------------------------
@pytest.mark.parametrize("alg,prim,sec", ALGS)
def test_hybrid_dv4_rows_in_lds(gpu_available, alg, prim, sec):
    bsc_parity("hybrid_dv4_lds", alg, prim, sec, 12)
    S.assert_plan(graph("hybrid_dv4_lds"), "hybrid_dv4_lds", alg)


@pytest.mark.parametrize("alg,prim,sec", ALGS[2:])
def test_hybrid_dv4_minsum_vn_phase_path(gpu_available, monkeypatch, alg, prim, sec):
    """QLDPC_VNG=0 (read per launch): min-sum through the VN phases and the
    kpos-ordered slot_meta2 instead of the bit gather, still without a stage."""
    monkeypatch.setenv("QLDPC_DIAG", "1")
    monkeypatch.setenv("QLDPC_VNG", "0")
    bsc_parity("hybrid_dv4_lds", alg, prim, sec, 12)
    bsc_parity("hybrid_dv4_lds", alg, prim, sec, 8, seed=2, max_it=2, thr_on=False)
    S.assert_plan(graph("hybrid_dv4_lds"), "hybrid_dv4_lds", alg)


@pytest.mark.parametrize("alg,prim,sec", ALGS)
def test_hybrid_dv4_rows_partly_global(gpu_available, alg, prim, sec):
    """Min-sum row aggregates of 7 of the 16 waves in global scratch."""
    bsc_parity("hybrid_dv4_global", alg, prim, sec, 12)
    if alg in (Q.OMSA, Q.AOMSA):
        for max_it in (1, 2):
            bsc_parity("hybrid_dv4_global", alg, prim, sec, 8, seed=2, max_it=max_it, thr_on=False)
    S.assert_plan(graph("hybrid_dv4_global"), "hybrid_dv4_global", alg)


# ---- split frames at the smallest part counts -----------------------------------------------------
@pytest.mark.parametrize("alg,prim,sec", ALGS)
def test_split_k4_all_algorithms(gpu_available, alg, prim, sec):
    bsc_parity("split_k4", alg, prim, sec, 9)
    S.assert_plan(graph("split_k4"), "split_k4", alg)


@pytest.mark.parametrize("batch", [1, 2])
@pytest.mark.parametrize("alg,prim,sec", [SPA, OMSA])
def test_split_k4_few_frames(gpu_available, alg, prim, sec, batch):
    # fewer frames than part groups: most groups draw no frame and leave
    bsc_parity("split_k4", alg, prim, sec, batch, seed=10 + batch, spread=False)
    S.assert_plan(graph("split_k4"), "split_k4", alg)


@pytest.mark.parametrize("case", ["split_k2_w8", "split_k2_w16"])
@pytest.mark.parametrize("alg,prim,sec", [SPA, OMSA, AOMSA])
def test_split_k2(gpu_available, case, alg, prim, sec):
    """K = 2, the smallest group group_sync forms: 8-wave and 16-wave parts,
    each with 12 scratch slots per lane."""
    bsc_parity(case, alg, prim, sec, 8)
    S.assert_plan(graph(case), case, alg)


@pytest.mark.parametrize("case", ["split_k2_w8", "split_k2_w16"])
@pytest.mark.parametrize("alg,prim,sec", [SPA, OMSA, AOMSA])
def test_split_k2_deferred_exit_edges(gpu_available, case, alg, prim, sec):
    """Iteration caps 1-3 (the last iteration a scan only) and, on the 8-wave
    parts, a frame without errors beside ordinary ones."""
    for max_it in (1, 2, 3):
        bsc_parity(case, alg, prim, sec, 4, seed=2, max_it=max_it)
    if case == "split_k2_w8":
        H = matrix(case)
        a, b, llr, s = frames(H, qber(case, alg), 4, 3)
        llr[0] = np.abs(llr[0]) * np.where(a[0] != 0, -1.0, 1.0)  # Bob == Alice
        out, (ob, oi, ok, op) = assert_parity(case, alg, prim, sec, llr, s)
        assert ok[0] == 1 and oi[0] <= 1
    S.assert_plan(graph(case), case, alg)


# ---- row structures --------------------------------------------------------------------------------
@pytest.mark.parametrize("thr_on", [True, False])
@pytest.mark.parametrize("alg,prim,sec", ALGS)
def test_degree1_rows(gpu_available, alg, prim, sec, thr_on):
    """Two checks of one bit each.  The oracle defines them: with the threshold
    off every SPA posterior of every frame is NaN, and min-sum posteriors
    reach DBL_MAX (a 1-edge row keeps min2 = DBL_MAX) — matched bitwise."""
    out, (ob, oi, ok, op) = bsc_parity("degree1_rows", alg, prim, sec, 12, thr_on=thr_on, spread=thr_on)
    if not thr_on and alg == Q.SPA:
        assert np.isnan(op).all()
    if not thr_on and alg in MINSUM:  # (the normalised family scales it by its factor)
        top = np.abs(op[~np.isnan(op)]).max()
        assert top in ((DBL_MAX,) if alg in (Q.OMSA, Q.AOMSA) else (prim * DBL_MAX, sec * DBL_MAX)), top
    S.assert_plan(graph("degree1_rows"), "degree1_rows", alg)


@pytest.mark.parametrize("alg,prim,sec", ALGS)
def test_many_short_rows(gpu_available, alg, prim, sec):
    """4000 rows of 1..8 edges on 4096 bits of degree 2: 8 slots per lane."""
    bsc_parity("short_rows", alg, prim, sec, 12)
    S.assert_plan(graph("short_rows"), "short_rows", alg)


@pytest.mark.parametrize("alg,prim,sec", ALGS)
def test_lanes_that_start_32_rows(gpu_available, alg, prim, sec):
    """Whole lanes of one-edge rows under a 32-slot deal: every bit of the
    lane's 32-bit syndrome mask is a row start."""
    bsc_parity("row_starts_32", alg, prim, sec, 12)
    bsc_parity("row_starts_32", alg, prim, sec, 12, seed=2, thr_on=False, spread=False)
    S.assert_plan(graph("row_starts_32"), "row_starts_32", alg)


@pytest.mark.parametrize("alg,prim,sec", ALGS)
def test_row_of_32_edges(gpu_available, alg, prim, sec):
    """The longest row V2 holds; the plan has 3 waves, an odd count."""
    bsc_parity("long_row32", alg, prim, sec, 12)
    S.assert_plan(graph("long_row32"), "long_row32", alg)


@pytest.mark.parametrize("alg,prim,sec", [SPA, OMSA])
@pytest.mark.parametrize("dc", [33, 40, 41])
def test_rows_beyond_32_edges_fall_back_to_v1(gpu_available, dc, alg, prim, sec):
    case = f"long_row{dc}"
    bsc_parity(case, alg, prim, sec, 12)
    assert graph(case).plan(0, alg)["variant"] == ("glb_lds" if dc == 41 else "reg_lds")
    S.assert_plan(graph(case), case, alg)


@pytest.mark.parametrize("thr_on", [True, False])
@pytest.mark.parametrize("alg,prim,sec", ALGS)
def test_bit_of_degree_300(gpu_available, alg, prim, sec, thr_on):
    """Bit 0 in 300 two-edge rows (the hybrid bit gather's chunk table does not
    take a degree >= 256; the VN phases run 300 deep), bits 301..399 isolated.
    The graph is a tree, so every frame stops within a few iterations whatever
    the QBER: no frame can reach the default cap, and caps 1 and 2 stand in
    for the frames that do."""
    for q, max_it, seed in ((0.03, CAP, 1), (0.1, CAP, 2), (0.1, 1, 3), (0.1, 2, 3)):
        _, _, llr, s = frames(matrix("degree300_bit"), q, 12, seed)
        assert_parity("degree300_bit", alg, prim, sec, llr, s, max_it=max_it, thr_on=thr_on)
    S.assert_plan(graph("degree300_bit"), "degree300_bit", alg)


@pytest.mark.parametrize("alg,prim,sec", [SPA, AOMSA])
def test_bit_of_degree_510(gpu_available, alg, prim, sec):
    """The largest bit degree accepted, beside a 500-row chain."""
    bsc_parity("degree510_bit", alg, prim, sec, 12)
    bsc_parity("degree510_bit", alg, prim, sec, 12, seed=2, max_it=2)
    S.assert_plan(graph("degree510_bit"), "degree510_bit", alg)


@pytest.mark.parametrize("alg,prim,sec", [SPA, OMSA])
@pytest.mark.parametrize("case", ["empty_row_first", "empty_row_last"])
def test_leading_and_trailing_empty_row(gpu_available, case, alg, prim, sec):
    """An empty check before the first / after the last row (v1, reg_lds).  Its
    syndrome bit is 0 in the even frames and 1 in the odd ones: no decision
    satisfies those, so they reach the cap with syndromes_match == 0."""
    H = matrix(case)
    row = 0 if case == "empty_row_first" else H.m - 1
    assert H.row_ptr[row + 1] == H.row_ptr[row]
    _, _, llr, s = frames(H, qber(case, alg), 12, 1)
    assert not s[:, row].any()
    s[1::2, row] = 1
    out, (ob, oi, ok, op) = assert_parity(case, alg, prim, sec, llr, s)
    assert (oi[1::2] == CAP).all() and not ok[1::2].any()
    assert (out.iterations[1::2] == CAP).all() and not out.synd_ok[1::2].any()
    assert int((oi[0::2] < CAP).sum()) >= 2  # and the even frames are not all lost
    assert_spread(alg, oi)
    S.assert_plan(graph(case), case, alg)


@pytest.mark.parametrize("alg,prim,sec", [SPA, OMSA])
@pytest.mark.parametrize("case", ["reg44_isolated", "split_k4_isolated"])
def test_isolated_bits_off_the_40_slot_shape(gpu_available, case, alg, prim, sec):
    """About 1 % of the bits taken out of (nearly) every row: isolated bits on
    the 44-slot register shape and in split frames (K = 3 with the edges
    that are left)."""
    H = matrix(case)
    assert int((np.diff(H.col_ptr) == 0).sum()) >= H.n // 200
    bsc_parity(case, alg, prim, sec, 12 if case == "reg44_isolated" else 9)
    S.assert_plan(graph(case), case, alg)
