"""Symmetric blind reconciliation's entries (Bob's selection, Alice's answer,
Bob's positions round) on a host-only graph, with and without a plan: the
symbols are bound, the argument checks answer in their documented order before
any device is touched, the host entries check the list and the positions, and
the numpy restatement of the selection order holds on a hand-written row."""
import ctypes
import math
import os

import numpy as np
import pytest

import qkd_ldpc_v_amd as Q
from conftest import load_fixture
from qkd_ldpc_v_amd import _lib, blind
from symmetric_ref import excluded, np_select

C1 = "c1_n1024_m220.alist"
EINVAL, EUNSUP = -1, -5
NEW = ["qldpc_select_positions_device", "qldpc_disclose_positions_device", "qldpc_reconcile_positions_round_device",
       "qldpc_select_positions_batch", "qldpc_disclose_positions_batch", "qldpc_reconcile_positions_round_batch"]
PUNCT, SHORT = [0, 5, 31, 32, 1023], [1, 63, 64, 1000]
N = 1024


def err():
    return Q.lib().qldpc_last_error()


def calls(g, plan, p, batch, n_list, first, count, cap, buf=None, stride=N):
    """The six entries with `buf` for every buffer: name -> (return code, last
    error).  The round entries pin n_disc = count positions."""
    L, gh = Q.lib(), (None if g is None else g.handle)
    ph, pp = (None if plan is None else plan.handle), (None if p is None else ctypes.byref(p))
    b = buf
    out = {}
    for name, fn in (
        ("select_device", lambda: L.qldpc_select_positions_device(gh, ph, 0, batch, b, n_list, b, first, count, b, cap,
                                                                  None)),
        ("disclose_device", lambda: L.qldpc_disclose_positions_device(gh, ph, 0, n_list, b, b, stride, b, cap, first,
                                                                      count, b, None)),
        ("round_device", lambda: L.qldpc_reconcile_positions_round_device(gh, ph, 0, pp, batch, b, b, b, n_list, b,
                                                                          count, b, cap, b, b, b, b, None, None)),
        ("select", lambda: L.qldpc_select_positions_batch(gh, ph, batch, b, n_list, b, first, count, b, cap)),
        ("disclose", lambda: L.qldpc_disclose_positions_batch(gh, ph, batch, n_list, b, b, stride, b, cap, first, count,
                                                              b)),
        ("round", lambda: L.qldpc_reconcile_positions_round_batch(gh, ph, pp, batch, b, b, b, n_list, b, count, b, cap,
                                                                  b, b, b, b, None)),
    ):
        rc = fn()
        out[name] = (rc, err() if rc else b"")
    return out


WITH_PARAMS = ("round_device", "round")
WITH_BATCH = ("select_device", "round_device", "select", "disclose", "round")
HOST = ("select", "disclose", "round")
DEVICE = ("select_device", "disclose_device", "round_device")


@pytest.fixture(scope="module")
def graph_plan():
    g = Q.Graph(load_fixture(C1), host_only=True)
    return g, g.rate_plan(PUNCT, SHORT)


def test_symmetric_symbols_are_bound():
    assert set(NEW) <= set(_lib.exported_symbols())
    for name in NEW:
        assert getattr(Q.lib(), name).argtypes is not None
    for method in ("select_positions", "disclose_positions", "reconcile_positions_round"):
        assert callable(getattr(Q.Graph, method)) and callable(getattr(Q.Graph, method + "_device"))
    assert callable(blind.symmetric_reconcile) and Q.symmetric_reconcile is blind.symmetric_reconcile
    assert Q.SELECT_MAX == 4096
    with open(os.path.join(os.path.dirname(os.path.dirname(_lib.LIB_PATH)), "include", "qkd_ldpc_hip.h")) as fh:
        assert "#define QLDPC_SELECT_MAX 4096" in fh.read()


def test_null_graph_comes_first(graph_plan):
    _, plan = graph_plan
    bad = Q.Params(Q.SPA, 50, True, -1.0).c()
    for name, (rc, msg) in calls(None, plan, bad, -1, -1, -1, -1, -1).items():
        assert rc == EINVAL and b"graph is NULL" in msg, name


@pytest.mark.parametrize("with_plan", [True, False], ids=["plan", "no plan"])
def test_checks_in_their_order(graph_plan, with_plan):
    g, plan = graph_plan
    plan = plan if with_plan else None
    good = Q.Params(Q.SPA, 50).c()
    # the parameters come before every count
    r = calls(g, plan, Q.Params(Q.SPA, 50, True, math.nan).c(), -1, -1, -1, -1, -1)
    for name in WITH_PARAMS:
        assert r[name] == (EINVAL, b"threshold must be > 0 when enabled"), name
    r = calls(g, plan, None, -1, -1, -1, -1, -1)
    for name in WITH_PARAMS:
        assert r[name] == (EINVAL, b"params is NULL"), name
    # batch < 0, then n_list < 0, n_list > batch, then the window
    r = calls(g, plan, good, -1, -1, -1, -1, -1)
    for name in WITH_BATCH:
        assert r[name] == (EINVAL, b"batch must be >= 0"), name
    assert r["disclose_device"] == (EINVAL, b"n_list must be >= 0")  # (it takes no batch)
    for name, (rc, msg) in calls(g, plan, good, 4, -1, -1, -1, -1).items():
        assert (rc, msg) == (EINVAL, b"n_list must be >= 0"), name
    r = calls(g, plan, good, 4, 5, -1, -1, -1)
    for name in WITH_BATCH:
        assert r[name] == (EINVAL, b"n_list must be <= batch"), name
    window = b"first and count must be >= 0 with first + count <= cap"
    for first, count, cap in ((0, -1, 8), (0, 9, 8), (0, 1, -1)):
        for name, (rc, msg) in calls(g, plan, good, 4, 4, first, count, cap).items():
            assert (rc, msg) == (EINVAL, window), (name, first, count, cap)
    big = 2**31 - 1  # (the sum is taken in 64 bits; the round entries take no `first`)
    for first, count, cap in ((-1, 1, 8), (5, 4, 8), (big, big, big)):
        r = calls(g, plan, good, 4, 4, first, count, cap)
        for name in ("select_device", "disclose_device", "select", "disclose"):
            assert r[name] == (EINVAL, window), (name, first, count, cap)
    r = calls(g, plan, good, 4, 4, 0, 4, 8, stride=N - 1)
    for name in ("disclose_device", "disclose"):
        assert r[name] == (EINVAL, b"ext_stride must be >= n"), name
    # n_list == 0 answers OK with NULL buffers, on a graph without any device, even beyond the select limit
    for count, cap in ((0, 0), (20, 40), (Q.SELECT_MAX + 1, 5000)):
        for name, (rc, _) in calls(g, plan, good, 4, 0, 0, count, cap).items():
            assert rc == 0, (name, count)
    # then the buffers
    for name, (rc, msg) in calls(g, plan, good, 4, 2, 0, 1, 8).items():
        assert rc == EINVAL and b"NULL" in msg and b"buffer" in msg, (name, msg)


def test_lookups_after_the_buffers(graph_plan):
    """With buffers given: the host entries check the list and the positions,
    then need a device; the device entries look up the plan and the graph on
    the device.  The select limit answers before any lookup."""
    g, plan = graph_plan
    good = Q.Params(Q.SPA, 50).c()
    zeros = np.zeros(8 * N, np.int64).view(np.int32)  # list = [0, 0]: a frame named twice; every position 0
    p = zeros.ctypes.data
    r = calls(g, plan, good, 4, 2, 0, 1, 8, p)
    for name in DEVICE:
        assert r[name] == (EINVAL, b"rate plan does not live on that device"), name
    for name in HOST:
        assert r[name] == (EINVAL, b"list names a frame twice"), name
    r = calls(g, None, good, 4, 2, 0, 1, 8, p)
    for name in DEVICE:
        assert r[name] == (EINVAL, b"graph does not live on that device"), name
    for pl in (plan, None):
        r = calls(g, pl, good, 4, 1, 0, 1, 8, p)
        for name in HOST:
            assert r[name][0] == EINVAL and b"host-only" in r[name][1], (name, r[name])
        r = calls(g, pl, good, 5000, 1, 0, Q.SELECT_MAX + 1, 5000, p)
        assert r["select_device"][0] == EUNSUP and b"QLDPC_SELECT_MAX" in r["select_device"][1]
    # the history of frame 0 is [0, 0]: a position named twice (select reads [0, first), the others [0, n_disc))
    r = calls(g, plan, good, 4, 1, 2, 1, 8, p)
    assert r["select"] == (EINVAL, b"pos names a position twice")
    r = calls(g, plan, good, 4, 1, 0, 2, 8, p)
    for name in ("disclose", "round"):
        assert r[name] == (EINVAL, b"pos names a position twice"), name
    zeros[0] = 4
    r = calls(g, plan, good, 4, 1, 0, 1, 8, p)
    for name in HOST:
        assert r[name] == (EINVAL, b"list names a frame outside [0, batch)"), name


def test_host_position_checks(graph_plan):
    """Through the wrappers: positions outside [0, n), and a count beyond the frame's candidates."""
    g, plan = graph_plan
    post = np.zeros((3, N))
    keys, syn = np.zeros((3, N), np.uint8), np.zeros((3, g.m), np.uint8)
    pos = np.full((3, N), -1, np.int32)
    pos[1, :3] = [7, N, 9]
    with pytest.raises(Q.QLDPCError, match=r"EINVAL.*outside \[0, n\)"):
        g.select_positions(post, [1], 3, 2, pos, plan=plan)
    with pytest.raises(Q.QLDPCError, match=r"EINVAL.*outside \[0, n\)"):
        g.disclose_positions(keys, [1], pos, 0, 3)
    with pytest.raises(Q.QLDPCError, match=r"EINVAL.*outside \[0, n\)"):  # (-1: a column that was never selected)
        g.reconcile_positions_round(Q.Params(Q.SPA, 50), keys, 3.5, syn, [0], 1, pos, np.zeros((1, 1), np.uint8))
    pos[1, :3] = [7, 8, 9]
    cands = N - len(SHORT) - 3
    with pytest.raises(Q.QLDPCError, match="EINVAL.*candidates"):
        g.select_positions(post, [1], 3, cands + 1, pos, plan=plan)
    with pytest.raises(Q.QLDPCError, match="EINVAL.*candidates"):  # without a plan the shortened ones count too
        g.select_positions(post, [1], 3, N - 3 + 1, np.full((3, 2 * N), 5, np.int32))
    for pl, count in ((plan, cands), (None, N - 3)):  # every candidate is a legal count: then the device is missed
        with pytest.raises(Q.QLDPCError, match="EINVAL.*host-only"):
            g.select_positions(post, [1], 3, count, pos.copy(), plan=pl)
    big = Q.Graph(Q.regular_code(6000, 3000, 3, seed=1), host_only=True)
    with pytest.raises(Q.QLDPCError, match="EUNSUP.*QLDPC_SELECT_MAX"):
        big.select_positions(np.zeros((1, 6000)), [0], 0, Q.SELECT_MAX + 1, np.full((1, 6000), -1, np.int32))


def test_wrappers_on_empty_lists(graph_plan):
    g, plan = graph_plan
    for pl in (plan, None):
        pos = np.full((3, 40), -1, np.int32)
        assert g.select_positions(np.zeros((3, N)), [], 0, 20, pos, plan=pl) is pos and (pos == -1).all()
        assert g.disclose_positions(np.zeros((3, N + 8), np.uint8), [], pos, 0, 20, plan=pl).shape == (0, 20)
        keys, syn = np.zeros((3, N), np.uint8), np.zeros((3, g.m), np.uint8)
        prev = Q.DecodeOutput(np.full((3, N), 7, np.uint8), np.full(3, 9, np.uint32), np.full(3, 1, np.uint8), None)
        out = g.reconcile_positions_round(Q.Params(Q.SPA, 50), keys, 3.5, syn, [], 20, pos, np.empty((0, 20), np.uint8),
                                          plan=pl, out=prev)
        assert out is prev and (out.bits == 7).all() and (out.iterations == 9).all() and (out.synd_ok == 1).all()
    with pytest.raises(ValueError, match="vals"):
        g.reconcile_positions_round(Q.Params(Q.SPA, 50), keys, 3.5, syn, [0, 1], 1, pos, np.zeros((2, 2), np.uint8))
    with pytest.raises(ValueError, match="int32"):
        g.select_positions(np.zeros((3, N)), [], 0, 20, pos.astype(np.int64))
    with pytest.raises(ValueError, match="plans differ"):
        Q.symmetric_reconcile(g, plan, g, None, Q.Params(Q.SPA, 20), keys, keys, 3.5)


def test_np_select_by_hand():
    """+-0 tie at the bottom, then a denormal, 1e-4, 1, DBL_MAX, inf, NaN; equal
    magnitudes go to the lower index whatever their signs."""
    dmax = np.finfo(np.float64).max
    row = np.array([1.0, -0.0, np.nan, 5e-324, -1.0, np.inf, 0.0, -1e-4, dmax, -np.inf, 1e-4, -dmax])
    order = [1, 6, 3, 7, 10, 0, 4, 8, 11, 5, 9, 2]
    none = excluded(row.size)
    assert np_select(row, none, row.size).tolist() == order
    for count in range(row.size + 1):  # a shorter selection is a prefix of a longer one
        assert np_select(row, none, count).tolist() == order[:count]
    # excluded positions (shortened ones, the history) are skipped and the rest keep their order
    assert np_select(row, excluded(row.size, [6, 0], [7, 3]), 5).tolist() == [1, 10, 4, 8, 11]
    assert np_select(row, none, 3).dtype == np.int32
    # the order is the integers', not the floats': a negative NaN with a payload sorts after a positive quiet NaN
    nans = np.array([0x7FF8000000000000, 0xFFF8000000000001, 0x7FF0000000000000], np.uint64).view(np.float64)
    assert np_select(nans, excluded(3), 3).tolist() == [2, 0, 1]
