"""Blind reconciliation's entries (failed-frame list, Alice's disclosure, Bob's
round) on a host-only graph and plan: the symbols are bound, the argument
checks answer in their documented order before any device is touched, and the
pure pieces of qkd_ldpc_v_amd.blind (efficiency, the disclosure order) hold."""
import ctypes
import math

import numpy as np
import pytest

import qkd_ldpc_v_amd as Q
from conftest import load_fixture
from qkd_ldpc_v_amd import _lib, blind

C1 = "c1_n1024_m220.alist"
EINVAL = -1
NEW = ["qldpc_failed_frames_device", "qldpc_disclose_device", "qldpc_reconcile_round_device", "qldpc_disclose_batch",
       "qldpc_reconcile_round_batch"]
PUNCT, SHORT = [0, 5, 31, 32, 1023], [1, 63, 64, 1000]


def err():
    return Q.lib().qldpc_last_error()


def calls(g, plan, p, batch, n_list, n_disc, buf=None):
    """The four graph entries with `buf` for every buffer: name -> (return code, last error)."""
    L, gh = Q.lib(), (None if g is None else g.handle)
    ph, pp = (None if plan is None else plan.handle), (None if p is None else ctypes.byref(p))
    b = buf
    out = {}
    for name, fn in (
        ("disclose_device", lambda: L.qldpc_disclose_device(gh, ph, 0, n_list, b, b, n_disc, b, b, None)),
        ("round_device", lambda: L.qldpc_reconcile_round_device(gh, ph, 0, pp, batch, b, b, b, n_list, b, n_disc, b, b,
                                                                b, b, b, None, None)),
        ("disclose", lambda: L.qldpc_disclose_batch(gh, ph, batch, n_list, b, b, n_disc, b, b)),
        ("round", lambda: L.qldpc_reconcile_round_batch(gh, ph, pp, batch, b, b, b, n_list, b, n_disc, b, b, b, b, b,
                                                        None)),
    ):
        rc = fn()
        out[name] = (rc, err() if rc else b"")
    return out


WITH_PARAMS = ("round_device", "round")
WITH_BATCH = ("round_device", "disclose", "round")


@pytest.fixture(scope="module")
def graph_plan():
    g = Q.Graph(load_fixture(C1), host_only=True)
    return g, g.rate_plan(PUNCT, SHORT)


def test_blind_symbols_are_bound():
    assert set(NEW) <= set(_lib.exported_symbols())
    for name in NEW:
        assert getattr(Q.lib(), name).argtypes is not None
    for method in ("failed_frames_device", "disclose", "disclose_device", "reconcile_round", "reconcile_round_device"):
        assert callable(getattr(Q.Graph, method))
    assert callable(blind.blind_reconcile) and Q.blind_reconcile is blind.blind_reconcile


def test_null_graph_comes_first(graph_plan):
    _, plan = graph_plan
    bad = Q.Params(Q.SPA, 50, True, -1.0).c()
    for name, (rc, msg) in calls(None, plan, bad, -1, -1, -1).items():
        assert rc == EINVAL and b"graph is NULL" in msg, name


def test_checks_in_their_order(graph_plan):
    g, plan = graph_plan
    good = Q.Params(Q.SPA, 50).c()
    # the parameters come before every count
    r = calls(g, plan, Q.Params(Q.SPA, 50, True, math.nan).c(), -1, -1, -1)
    for name in WITH_PARAMS:
        assert r[name] == (EINVAL, b"threshold must be > 0 when enabled"), name
    r = calls(g, plan, None, -1, -1, -1)
    for name in WITH_PARAMS:
        assert r[name] == (EINVAL, b"params is NULL"), name
    # batch < 0, then n_list < 0, n_list > batch, then n_disc outside [0, n_punct]
    r = calls(g, plan, good, -1, -1, -1)
    for name in WITH_BATCH:
        assert r[name] == (EINVAL, b"batch must be >= 0"), name
    assert r["disclose_device"] == (EINVAL, b"n_list must be >= 0")  # (it takes no batch)
    for name, (rc, msg) in calls(g, plan, good, 4, -1, -1).items():
        assert (rc, msg) == (EINVAL, b"n_list must be >= 0"), name
    r = calls(g, plan, good, 4, 5, -1)
    for name in WITH_BATCH:
        assert r[name] == (EINVAL, b"n_list must be <= batch"), name
    for n_disc in (-1, len(PUNCT) + 1):
        for name, (rc, msg) in calls(g, plan, good, 4, 4, n_disc).items():
            assert (rc, msg) == (EINVAL, b"n_disc must be in [0, n_punct]"), (name, n_disc)
    # n_list == 0 answers OK with NULL buffers and no plan, on a graph without any device
    for pl in (plan, None):
        for n_disc in (0, len(PUNCT)):
            for name, (rc, _) in calls(g, pl, good, 4, 0, n_disc).items():
                assert rc == 0, (name, n_disc)
    # then the plan, then the buffers
    for name, (rc, msg) in calls(g, None, good, 4, 2, 1).items():
        assert (rc, msg) == (EINVAL, b"plan is NULL"), name
    for name, (rc, msg) in calls(g, plan, good, 4, 2, 1).items():
        assert rc == EINVAL and b"NULL" in msg and b"buffer" in msg, (name, msg)


def test_lookups_after_the_buffers(graph_plan):
    """With buffers given: the host entries check the list and the indices,
    then need a device; the device entries look up the plan on the device."""
    g, plan = graph_plan
    good = Q.Params(Q.SPA, 50).c()
    zeros = np.zeros(8 * 1024, np.int32)  # list = [0, 0]: a frame named twice (never read as anything else)
    r = calls(g, plan, good, 4, 2, 1, zeros.ctypes.data)
    for name in ("disclose_device", "round_device"):
        assert r[name] == (EINVAL, b"rate plan does not live on that device"), name
    for name in ("disclose", "round"):
        assert r[name] == (EINVAL, b"list names a frame twice"), name
    r = calls(g, plan, good, 4, 1, 1, zeros.ctypes.data)
    for name in ("disclose", "round"):
        assert r[name][0] == EINVAL and b"host-only" in r[name][1], name
    zeros[0] = 4
    r = calls(g, plan, good, 4, 1, 1, zeros.ctypes.data)
    for name in ("disclose", "round"):
        assert r[name] == (EINVAL, b"list names a frame outside [0, batch)"), name
    zeros[0] = len(PUNCT)  # list = [5] of 8 frames is fine; disc = [5] of 5 punctured is not
    r = calls(g, plan, good, 8, 1, 1, zeros.ctypes.data)
    for name in ("disclose", "round"):
        assert r[name] == (EINVAL, b"disc names an index outside [0, n_punct)"), name


def test_failed_list_entry_checks():
    L = Q.lib()
    assert L.qldpc_failed_frames_device(-1, None, None, None, None) == EINVAL and b"batch must be >= 0" in err()
    assert L.qldpc_failed_frames_device(0, None, None, None, None) == 0  # nothing to list, no device touched
    assert L.qldpc_failed_frames_device(3, None, None, None, None) == EINVAL and b"NULL device buffer" in err()


def test_wrappers_on_empty_lists(graph_plan):
    g, plan = graph_plan
    H = g.H
    fill = np.zeros((3, len(PUNCT)), np.uint8)
    assert g.disclose(plan, [], fill, [0, 1]).shape == (0, 2)
    keys, syn = np.zeros((3, H.n), np.uint8), np.zeros((3, H.m), np.uint8)
    prev = Q.DecodeOutput(np.full((3, H.n), 7, np.uint8), np.full(3, 9, np.uint32), np.full(3, 1, np.uint8), None)
    out = g.reconcile_round(Q.Params(Q.SPA, 50), keys, 3.5, syn, plan, [], [0], np.empty((0, 1), np.uint8), out=prev)
    assert out is prev and (out.bits == 7).all() and (out.iterations == 9).all() and (out.synd_ok == 1).all()
    with pytest.raises(ValueError, match="rate plan"):
        g.disclose(None, [0], fill, [0])
    with pytest.raises(ValueError, match="vals"):
        g.reconcile_round(Q.Params(Q.SPA, 50), keys, 3.5, syn, plan, [0, 1], [0], np.zeros((2, 2), np.uint8))
    with pytest.raises(Q.QLDPCError, match="EINVAL.*host-only"):
        g.reconcile_round(Q.Params(Q.SPA, 50), keys, 3.5, syn, plan, [0, 1], [0], np.zeros((2, 1), np.uint8))


def test_efficiency_by_hand():
    """C1 with 60 punctured and 4 shortened positions at q = 0.016:
    (220 - 60 + d) / ((1024 - 64) h2(0.016))."""
    q = 0.016
    h2 = -(q * math.log2(q) + (1 - q) * math.log2(1 - q))
    assert blind.h2(q) == pytest.approx(h2, rel=1e-15) and 0.11 < h2 < 0.12
    got = blind.blind_efficiency(1024, 220, 60, 4, np.array([0, 20, 60]), q)
    want = np.array([160.0, 180.0, 220.0]) / (960 * h2)
    assert got.dtype == np.float64 and np.allclose(got, want, rtol=1e-14, atol=0)
    assert np.allclose(got, [1.4083, 1.5843, 1.9363], atol=5e-4)  # h2 = 0.11835: 160, 180, 220 over 113.616 bits
    assert np.isnan(blind.blind_efficiency(1024, 220, 60, 4, np.array([0, 20]), None)).all()
    assert Q.blind_efficiency(1024, 220, 60, 4, 20, q) == pytest.approx(180 / (960 * h2))


def test_order_must_be_a_permutation(graph_plan):
    g, plan = graph_plan
    assert np.array_equal(blind.check_order(None, 5), np.arange(5))
    assert np.array_equal(blind.check_order([4, 0, 3, 1, 2], 5), [4, 0, 3, 1, 2])
    H = g.H
    keys, fill = np.zeros((2, H.n), np.uint8), np.zeros((2, len(PUNCT)), np.uint8)
    for bad in ([0, 1, 2, 3], [0, 1, 2, 3, 3], [0, 1, 2, 3, 5], [-1, 0, 1, 2, 3], [0.0, 1.0, 2.0, 3.0, 4.0],
                [[0, 1, 2, 3, 4]]):
        with pytest.raises(ValueError, match="permutation"):  # (before anything is computed: the graph has no device)
            Q.blind_reconcile(g, plan, g, plan, Q.Params(Q.SPA, 20), keys, keys, 3.5, fill, 2, order=bad)
