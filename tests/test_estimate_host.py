"""Error estimation at the reconciliation stage, the host side: the degree
classes (qldpc_estimate_classes) and the solver (qldpc_qber_from_weight)
against tests/estimate_ref.py on host-only graphs, the bounds, the argument
order of every new entry, and the definition itself against the binomial law."""
import ctypes
import gzip
import math

import numpy as np
import pytest

import estimate_ref as R
import qkd_ldpc_v_amd as Q
from conftest import load_fixture, matrix_path
from qkd_ldpc_v_amd import _lib

C1, C2 = "c1_n1024_m220.alist", "c2_n10240_m2201.alist"
EINVAL = -1
NEW = ["qldpc_estimate_classes", "qldpc_qber_from_weight", "qldpc_estimate_qber_device", "qldpc_estimate_qber_batch",
       "qldpc_corrected_errors_device", "qldpc_corrected_errors_batch"]
# the blind fixture's plan (tests/test_gpu_blind.py): 60 punctured, 4 shortened
BLIND_PUNCT = np.arange(5, 1024, 16)[:60].astype(np.int32)
BLIND_PUNCT[0], BLIND_PUNCT[-1] = 0, 1023
BLIND_PUNCT = np.unique(BLIND_PUNCT)
BLIND_SHORT = np.array([1, 63, 64, 1000], np.int32)


def err():
    return Q.lib().qldpc_last_error()


def u64(x):
    return np.asarray(x, np.float64).view(np.uint64)


def host_graph(name):
    return Q.Graph(load_fixture(name), host_only=True)


def c2_plan_lists():
    pos = np.random.Generator(np.random.PCG64(1810)).permutation(10240)[:200]
    return np.sort(pos[:100]).astype(np.int32), np.sort(pos[100:]).astype(np.int32)


def row_of(H, j):
    return np.asarray(H.col_idx[H.row_ptr[j]:H.row_ptr[j + 1]], np.int32)


def u_plans():
    """On u_n10_m5: a plan that shortens every neighbour of row 0 (d = 0: not
    informative), and one whose punctured positions touch every row."""
    H = load_fixture("u_n10_m5.dense")
    short = np.unique(row_of(H, 0))
    taint = np.unique([row_of(H, j)[0] for j in range(H.m)]).astype(np.int32)
    return short, taint


CASES = [("kat_n6_m4.dense", None, None), ("u_n10_m5.dense", None, None), ("s1_n10_m5.sp1", None, None),
         (C1, None, None), (C1, BLIND_PUNCT, BLIND_SHORT), (C2, *c2_plan_lists()),
         ("m2k_n10240_m1024.sp2", "untp", None), ("u_n10_m5.dense", None, "row0")]


@pytest.mark.parametrize("name,punct,short", CASES, ids=[f"{c[0]}-{i}" for i, c in enumerate(CASES)])
def test_classes_match_the_reference(name, punct, short):
    H = load_fixture(name)
    if isinstance(punct, str):  # the fixture's own list as punctured positions
        punct = np.sort(np.array(gzip.open(matrix_path(name.replace(".sp2", ".untp"))).read().split(), np.int32))
        assert punct.size > 0
    if isinstance(short, str):
        short = u_plans()[0]
    g = Q.Graph(H, host_only=True)
    plan = None if punct is None and short is None else g.rate_plan([] if punct is None else punct,
                                                                    [] if short is None else short)
    deg, rows = g.estimate_classes(plan)
    D = R.dense(H)
    wd, wr = R.classes(D, punct, short)
    assert deg.dtype == np.int32 and np.array_equal(deg, wd) and np.array_equal(rows, wr)
    assert np.all(np.diff(deg) > 0) and np.all(deg >= 1)
    assert int(rows.sum()) == int((R.row_degrees(D, punct, short) > 0).sum())
    assert np.array_equal(R.row_degrees(D, punct, short), R.row_degrees_csr(H, punct, short))
    if plan is None:
        assert int(rows.sum()) == int((np.diff(H.row_ptr) >= 1).sum())
    if name == C2 and plan is not None:
        assert int(rows.sum()) < H.m  # (about 1835 of 2201 rows stay informative under such a draw)
    if isinstance(short, np.ndarray) and name.startswith("u_"):
        assert R.row_degrees(D, punct, short)[0] == 0 and int(rows.sum()) < H.m
    # a short output takes the first classes and still reports the count
    cnt = ctypes.c_int32(-1)
    one_d, one_r = np.full(1, -7, np.int32), np.full(1, -7, np.int32)
    ph = None if plan is None else plan.handle
    assert Q.lib().qldpc_estimate_classes(g.handle, ph, 1, ctypes.byref(cnt), one_d.ctypes.data, one_r.ctypes.data) == 0
    assert cnt.value == deg.size and (deg.size == 0 or (one_d[0], one_r[0]) == (deg[0], rows[0]))


def test_no_informative_rows_is_refused():
    g = host_graph("u_n10_m5.dense")
    plan = g.rate_plan(u_plans()[1], [])
    deg, rows = g.estimate_classes(plan)
    assert deg.size == 0 and rows.size == 0
    with pytest.raises(Q.QLDPCError, match="EINVAL.*no informative rows"):
        g.qber_from_weight([0], plan)
    L, buf = Q.lib(), np.zeros(64, np.uint8).ctypes.data
    assert L.qldpc_estimate_qber_device(g.handle, plan.handle, 0, 1, buf, buf, 0.01, 0.2, buf, None, None, None) == EINVAL
    assert b"no informative rows" in err()
    assert L.qldpc_estimate_qber_batch(g.handle, plan.handle, 1, buf, buf, 0.01, 0.2, buf, None, None) == EINVAL
    assert b"no informative rows" in err()


def solver_cases():
    p2, s2 = c2_plan_lists()
    return [(C1, None, None, None), (C1, BLIND_PUNCT, BLIND_SHORT, None), (C2, None, None, 200), (C2, p2, s2, 200)]


@pytest.mark.parametrize("name,punct,short,count", solver_cases(), ids=["c1", "c1-plan", "c2", "c2-plan"])
def test_solver_is_bit_identical(name, punct, short, count):
    g = host_graph(name)
    plan = None if punct is None else g.rate_plan(punct, short)
    deg, cnt = R.classes(R.dense(g.H), punct, short)
    rows = int(cnt.sum())
    ks = np.arange(rows + 1) if count is None else np.unique(np.linspace(0, rows, count).astype(np.int64))
    assert ks[0] == 0 and ks[-1] == rows
    q_min, q_max = 1e-4, 0.25
    q, lp = g.qber_from_weight(ks, plan, q_min, q_max)
    want = np.array([R.qber(deg, cnt, k, q_min, q_max) for k in ks])
    assert np.array_equal(u64(q), u64(want)), "q differs from the Python-float restatement"
    assert np.array_equal(u64(lp), u64([math.log1p((1.0 - 2.0 * x) / x) for x in q])), "log_p is not log1p((1-2q)/q)"
    assert np.all(np.diff(q) >= 0), "q must not fall as the weight rises"
    assert q[0] == q_min and q[-1] == q_max, "both clamps are reached exactly"
    assert np.all((q >= q_min) & (q <= q_max)) and np.unique(q).size > ks.size // 4
    assert np.all(np.isfinite(lp)) and np.all(lp > 0)


def test_pooled_weights():
    g = host_graph(C1)
    deg, cnt = R.classes(R.dense(g.H))
    sums = np.array([0, 7, 200, 371, 7 * 40, 7 * 100, 7 * 220], np.int64)
    q, lp = g.qber_from_weight(sums, None, 1e-3, 0.3, frames_per_weight=7)
    want = [R.qber(deg, cnt, k, 1e-3, 0.3, frames=7) for k in sums]
    assert np.array_equal(u64(q), u64(want))
    assert np.array_equal(u64(lp), u64([R.log_p(x) for x in want]))
    # seven equal frames: the pooled root is the per-frame root up to the bisection's last steps
    one, _ = g.qber_from_weight([40], None, 1e-3, 0.3)
    assert abs(q[4] - one[0]) < 1e-12
    with pytest.raises(Q.QLDPCError, match="EINVAL.*outside"):
        g.qber_from_weight([7 * 220 + 1], None, 1e-3, 0.3, frames_per_weight=7)
    with pytest.raises(Q.QLDPCError, match="EINVAL.*outside"):
        g.qber_from_weight([-1])
    with pytest.raises(Q.QLDPCError, match="EINVAL.*frames_per_weight"):
        g.qber_from_weight([1], frames_per_weight=0)
    # no log_p output
    w, out = np.array([40], np.int64), np.zeros(1)
    assert Q.lib().qldpc_qber_from_weight(g.handle, None, 1, w.ctypes.data, 1, 1e-3, 0.3, out.ctypes.data, None) == 0
    assert out[0] == one[0]


BAD_BOUNDS = [(0.0, 0.2), (-0.1, 0.2), (0.01, 0.5), (0.01, 0.7), (0.2, 0.1), (math.nan, 0.2), (0.01, math.nan)]


@pytest.mark.parametrize("q_min,q_max", BAD_BOUNDS)
def test_bounds(q_min, q_max):
    g = host_graph(C1)
    with pytest.raises(Q.QLDPCError, match="EINVAL.*0 < q_min <= q_max < 0.5"):
        g.qber_from_weight([3], None, q_min, q_max)
    L, buf = Q.lib(), np.zeros(4096, np.uint8).ctypes.data
    # the device and host-buffer entries: after the buffers, before any device is looked up
    assert L.qldpc_estimate_qber_device(g.handle, None, 0, 1, buf, buf, q_min, q_max, None, buf, None, None) == EINVAL
    assert b"q_min" in err()
    assert L.qldpc_estimate_qber_batch(g.handle, None, 1, buf, buf, q_min, q_max, None, None, buf) == EINVAL
    assert b"q_min" in err()
    # weights alone: nothing is solved and the bounds are not looked at (the device is, and is missing)
    assert L.qldpc_estimate_qber_device(g.handle, None, 0, 1, buf, buf, q_min, q_max, buf, None, None, None) == EINVAL
    assert b"graph does not live" in err()


def test_equal_bounds_and_the_widest_window():
    g = host_graph(C1)
    q, lp = g.qber_from_weight([0, 50, 220], None, 0.02, 0.02)
    assert np.all(q == 0.02) and np.array_equal(u64(lp), u64([R.log_p(0.02)] * 3))
    tiny, top = 1e-300, math.nextafter(0.5, 0.0)
    deg, cnt = R.classes(R.dense(g.H))
    q, lp = g.qber_from_weight([0, 1, 60, 110, 220], None, tiny, top)
    assert np.array_equal(u64(q), u64([R.qber(deg, cnt, k, tiny, top) for k in (0, 1, 60, 110, 220)]))
    assert np.all((q > 0) & (q < 0.5)) and np.all(np.isfinite(lp)) and np.all(lp > 0)


# ---- the argument order of every new entry ----------------------------------------
def calls(g, plan, batch, q=(0.01, 0.2)):
    L, gh = Q.lib(), (None if g is None else g.handle)
    ph = None if plan is None else plan.handle
    out = {}
    for name, fn in (
        ("from_weight", lambda: L.qldpc_qber_from_weight(gh, ph, batch, None, 1, q[0], q[1], None, None)),
        ("estimate_device", lambda: L.qldpc_estimate_qber_device(gh, ph, 0, batch, None, None, q[0], q[1], None, None,
                                                                 None, None)),
        ("estimate", lambda: L.qldpc_estimate_qber_batch(gh, ph, batch, None, None, q[0], q[1], None, None, None)),
        ("errors_device", lambda: L.qldpc_corrected_errors_device(gh, ph, 0, batch, None, None, None, None)),
        ("errors", lambda: L.qldpc_corrected_errors_batch(gh, ph, batch, None, None, None)),
    ):
        rc = fn()
        out[name] = (rc, err() if rc else b"")
    return out


@pytest.fixture(scope="module", params=["plain", "plan"])
def graph_plan(request):
    g = host_graph(C1)
    return g, (g.rate_plan(BLIND_PUNCT, BLIND_SHORT) if request.param == "plan" else None)


def test_symbols_are_bound():
    assert set(NEW) <= set(_lib.exported_symbols())
    for name in NEW:
        assert getattr(Q.lib(), name).argtypes is not None
    for method in ("estimate_classes", "qber_from_weight", "estimate_qber", "estimate_qber_device", "corrected_errors",
                   "corrected_errors_device"):
        assert callable(getattr(Q.Graph, method))
    assert Q.estimate.prior and Q.estimate.corrected_errors and Q.estimate.block_qber and Q.estimate.Tracker


def test_argument_order(graph_plan):
    g, plan = graph_plan
    for name, (rc, msg) in calls(None, plan, -1, (0.0, 0.9)).items():  # the graph comes first
        assert rc == EINVAL and b"graph is NULL" in msg, name
    cnt = ctypes.c_int32()
    assert Q.lib().qldpc_estimate_classes(None, None, 0, ctypes.byref(cnt), None, None) == EINVAL
    assert b"graph is NULL" in err()
    for name, (rc, msg) in calls(g, plan, -1, (0.0, 0.9)).items():  # then the batch, before the bounds
        assert rc == EINVAL and (b"batch" in msg or b"count" in msg), name
    for name, (rc, _) in calls(g, plan, 0, (0.0, 0.9)).items():  # an empty batch: OK, nothing looked at
        assert rc == 0, name
    for name, (rc, msg) in calls(g, plan, 2, (0.0, 0.9)).items():  # NULL buffers before the bounds
        assert rc == EINVAL and b"NULL" in msg and b"buffer" in msg, (name, msg)
    # buffers given: the bounds, then the plan on the device / the device
    L, H = Q.lib(), g.H
    buf = np.zeros(4 * H.n, np.uint8).ctypes.data  # (never read: the lookups fail first)
    ph = None if plan is None else plan.handle
    want = b"graph does not live" if plan is None else b"rate plan does not live"
    assert L.qldpc_estimate_qber_device(g.handle, ph, 0, 2, buf, buf, 0.0, 0.2, buf, buf, buf, None) == EINVAL
    assert b"q_min" in err()
    assert L.qldpc_estimate_qber_device(g.handle, ph, 0, 2, buf, buf, 0.01, 0.2, buf, buf, buf, None) == EINVAL
    assert want in err()
    assert L.qldpc_corrected_errors_device(g.handle, ph, 0, 2, buf, buf, buf, None) == EINVAL and want in err()
    keys = np.zeros((2, H.n), np.uint8)
    with pytest.raises(Q.QLDPCError, match="EINVAL.*host-only"):
        g.estimate_qber(keys, np.zeros((2, H.m), np.uint8), plan)
    with pytest.raises(Q.QLDPCError, match="EINVAL.*host-only"):
        g.corrected_errors(keys, keys, plan)
    with pytest.raises(ValueError, match="syndrome"):
        g.estimate_qber(keys, np.zeros((2, H.m + 1), np.uint8), plan)
    with pytest.raises(ValueError, match="bits"):
        g.corrected_errors(keys, np.zeros((2, H.n + 1), np.uint8), plan)


def test_a_plan_of_another_graph_is_refused():
    g1, g2 = host_graph(C1), host_graph("u_n10_m5.dense")
    plan = g2.rate_plan([], [3])
    with pytest.raises(Q.QLDPCError, match="EINVAL.*another adjacency"):
        g1.estimate_classes(plan)
    with pytest.raises(Q.QLDPCError, match="EINVAL.*another adjacency"):
        g1.qber_from_weight([1], plan)
    same = host_graph(C1)  # a second graph of the same matrix takes the plan
    assert np.array_equal(same.estimate_classes(g1.rate_plan(BLIND_PUNCT, BLIND_SHORT))[1],
                          g1.estimate_classes(g1.rate_plan(BLIND_PUNCT, BLIND_SHORT))[1])


def test_block_qber_and_tracker():
    E = Q.estimate
    assert E.block_qber([3, 100, 5, 0], 960, [0, 2, 3]) == 8 / (3 * 960)
    assert E.block_qber([3, 100], 960, []) == 0.0
    t = E.Tracker(0.25, 0.02)
    assert t.update(0.04) == 0.25 * 0.04 + 0.75 * 0.02 and t.q == 0.25 * 0.04 + 0.75 * 0.02
    assert E.Tracker(1.0, 0.3).update(0.01) == 0.01 and E.Tracker(0.0, 0.3).update(0.01) == 0.3
    with pytest.raises(ValueError):
        E.Tracker(1.5, 0.02)


# ---- the definition itself: the reference against the binomial law -------------------
def test_reference_estimator_within_five_sigma():
    """C2 without a plan, 64 frames with exactly floor(n q) flips at q = 0.0215:
    every estimate lies within 5 sigma of floor(n q) / n, sigma =
    sqrt(p (1 - p) / R) / (d (1 - 2q)^(d - 1)) with p = (1 - (1 - 2q)^d) / 2 and
    d the mean informative degree (the delta method on the binomial weight)."""
    H = load_fixture(C2)
    D = R.dense(H)
    deg, cnt = R.classes(D)
    rows, q = int(cnt.sum()), 0.0215
    flips = int(H.n * q)
    rng = np.random.Generator(np.random.PCG64(20181005))
    err_bits = np.zeros((64, H.n), np.uint8)
    for f in range(64):
        err_bits[f, rng.choice(H.n, flips, replace=False)] = 1
    # Bob = Alice + errors: the difference syndrome is H * errors whatever Alice holds
    alice = rng.integers(0, 2, (64, H.n), dtype=np.uint8)
    est, _, w = R.estimate(D, alice ^ err_bits, H.syndrome(alice))
    assert np.array_equal(w, ((err_bits.astype(np.int64) @ D.T.astype(np.int64)) & 1).sum(axis=1))
    dbar = float((deg * cnt).sum()) / rows
    p = (1.0 - (1.0 - 2.0 * q) ** dbar) / 2.0
    sigma = math.sqrt(p * (1.0 - p) / rows) / (dbar * (1.0 - 2.0 * q) ** (dbar - 1.0))
    dev = np.abs(est - flips / H.n)
    print(f"sigma {sigma:.6f}, worst deviation {dev.max() / sigma:.2f} sigma, mean error {np.mean(est - flips / H.n):+.2e}")
    assert np.all(dev <= 5.0 * sigma), (dev.max(), sigma)
