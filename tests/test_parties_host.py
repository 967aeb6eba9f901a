"""The per-party entries (Alice's syndromes, Bob's reconcile, key extraction) on
host-only graphs: the symbols are bound, and the argument checks that come
before any device is touched answer in their documented order (NULL graph,
parameters, batch < 0, batch == 0), with and without a rate plan."""
import ctypes
import math

import numpy as np
import pytest

import qkd_ldpc_v_amd as Q
from conftest import load_fixture
from qkd_ldpc_v_amd import _lib

C1 = "c1_n1024_m220.alist"
EINVAL = -1
NEW = ["qldpc_syndrome_batch_device", "qldpc_reconcile_batch_device", "qldpc_extract_key_device",
       "qldpc_syndrome_batch", "qldpc_reconcile_batch"]
PUNCT, SHORT = [0, 5, 31, 32, 1023], [1, 63, 64, 1000]


def err():
    return Q.lib().qldpc_last_error()


def calls(g, plan, p, batch):
    """Every new entry with NULL buffers: name -> return code, last error."""
    L, gh = Q.lib(), (None if g is None else g.handle)
    ph, pp = (None if plan is None else plan.handle), (None if p is None else ctypes.byref(p))
    out = {}
    for name, fn in (
        ("syndrome_device", lambda: L.qldpc_syndrome_batch_device(gh, ph, 0, batch, None, None, None, None, None)),
        ("reconcile_device", lambda: L.qldpc_reconcile_batch_device(gh, ph, 0, pp, batch, None, None, None, None,
                                                                    None, None, None, None, None)),
        ("extract_device", lambda: L.qldpc_extract_key_device(gh, ph, 0, batch, None, None, None)),
        ("syndrome", lambda: L.qldpc_syndrome_batch(gh, ph, batch, None, None, None, None)),
        ("reconcile", lambda: L.qldpc_reconcile_batch(gh, ph, pp, batch, None, None, None, None, None, None, None)),
    ):
        rc = fn()
        out[name] = (rc, err() if rc else b"")
    return out


@pytest.fixture(scope="module", params=["plain", "plan"])
def graph_plan(request):
    g = Q.Graph(load_fixture(C1), host_only=True)
    return g, (g.rate_plan(PUNCT, SHORT) if request.param == "plan" else None)


def test_party_symbols_are_bound():
    assert set(NEW) <= set(_lib.exported_symbols())
    for name in NEW:
        assert getattr(Q.lib(), name).argtypes is not None
    for method in ("syndrome", "reconcile", "syndrome_device", "reconcile_device", "extract_key_device"):
        assert callable(getattr(Q.Graph, method))


def test_null_graph_comes_first(graph_plan):
    _, plan = graph_plan
    bad = Q.Params(Q.SPA, 50, True, -1.0).c()  # (the graph is looked at before the parameters)
    for name, (rc, msg) in calls(None, plan, bad, -1).items():
        assert rc == EINVAL and b"graph is NULL" in msg, name


def test_parameters_then_batch(graph_plan):
    g, plan = graph_plan
    for thr in (0.0, -1.0, math.nan):
        r = calls(g, plan, Q.Params(Q.SPA, 50, True, thr).c(), -1)
        for name in ("reconcile_device", "reconcile"):
            assert r[name][0] == EINVAL and b"threshold must be > 0" in r[name][1], name
        for name in ("syndrome_device", "extract_device", "syndrome"):  # (no parameters: the batch)
            assert r[name][0] == EINVAL and b"batch" in r[name][1], name
    for name, (rc, msg) in calls(g, plan, Q.Params(Q.SPA, 50).c(), -1).items():
        assert rc == EINVAL and b"batch" in msg, name
    r = calls(g, plan, None, 0)  # NULL parameters
    for name in ("reconcile_device", "reconcile"):
        assert r[name][0] == EINVAL and b"params is NULL" in r[name][1], name


def test_empty_batch_touches_nothing(graph_plan):
    """batch == 0 answers OK with NULL buffers, on a graph without any device
    (and, for the extract entry, before the plan is asked for)."""
    g, plan = graph_plan
    for name, (rc, _) in calls(g, plan, Q.Params(Q.AOMSA, 7, True, 100.0, 0.55, 1.2).c(), 0).items():
        assert rc == 0, name


def test_wrappers_return_shaped_empty_outputs(graph_plan):
    g, plan = graph_plan
    H = g.H
    keys = np.empty((0, H.n), np.uint8)
    if plan is None:
        s = g.syndrome(keys)
    else:
        assert plan.n_key == H.n - len(PUNCT) - len(SHORT)
        ext, s = g.syndrome(keys, plan, np.empty((0, len(PUNCT)), np.uint8))
        assert ext.shape == (0, H.n) and ext.dtype == np.uint8
        ext2, s2 = g.syndrome(np.empty((0, plan.n_key), np.uint8), plan, np.empty((0, len(PUNCT)), np.uint8))
        assert ext2.shape == (0, H.n) and s2.shape == (0, H.m)
        with pytest.raises(ValueError, match="punct_fill"):
            g.syndrome(keys, plan)
    assert s.shape == (0, H.m) and s.dtype == np.uint8
    out = g.reconcile(Q.Params(Q.SPA, 50), keys, 3.5, np.empty((0, H.m), np.uint8), plan=plan, posterior=True)
    assert out.bits.shape == (0, H.n) and out.iterations.shape == (0,) and out.synd_ok.shape == (0,)
    assert out.iterations.dtype == np.uint32 and out.posterior.shape == (0, H.n)
    assert g.reconcile(Q.Params(Q.SPA, 50), keys, np.empty(0), np.empty((0, H.m), np.uint8), plan=plan).posterior is None
    with pytest.raises(ValueError, match="keys"):
        g.syndrome(np.empty((0, H.n + 1), np.uint8), plan, np.empty((0, len(PUNCT)), np.uint8))
    with pytest.raises(ValueError, match="syndrome"):
        g.reconcile(Q.Params(Q.SPA, 50), keys, 3.5, np.empty((0, H.m + 1), np.uint8), plan=plan)
    with pytest.raises(Q.QLDPCError, match="EINVAL.*threshold must be > 0"):
        g.reconcile(Q.Params(Q.SPA, 50, True, 0.0), keys, 3.5, np.empty((0, H.m), np.uint8), plan=plan)


def test_host_entries_need_a_device(graph_plan):
    """batch > 0: NULL buffers are refused first, then a graph without devices."""
    g, plan = graph_plan
    H = g.H
    for name, (rc, msg) in calls(g, plan, Q.Params(Q.SPA, 50).c(), 2).items():
        if name == "extract_device" and plan is None:
            assert rc == EINVAL and b"plan is NULL" in msg
        else:
            assert rc == EINVAL and b"NULL" in msg and b"buffer" in msg, (name, msg)
    keys = np.zeros((2, H.n), np.uint8)
    fill = np.zeros((2, len(PUNCT)), np.uint8)
    with pytest.raises(Q.QLDPCError, match="EINVAL.*host-only") as e:
        g.syndrome(keys, plan, fill if plan is not None else None)
    assert e.value.code == EINVAL
    with pytest.raises(Q.QLDPCError, match="EINVAL.*host-only") as e:
        g.reconcile(Q.Params(Q.SPA, 50), keys, 3.5, np.zeros((2, H.m), np.uint8), plan=plan)
    assert e.value.code == EINVAL
    # the device entries: the plan, then the graph, is looked up on the device
    L = Q.lib()
    buf = np.zeros(4 * H.n, np.uint8).ctypes.data  # (never read: the lookups fail first)
    p = Q.Params(Q.SPA, 50).c()
    ph = None if plan is None else plan.handle
    want = b"graph does not live" if plan is None else b"rate plan does not live"
    assert L.qldpc_syndrome_batch_device(g.handle, ph, 0, 2, buf, buf, None, buf, None) == EINVAL and want in err()
    assert L.qldpc_reconcile_batch_device(g.handle, ph, 0, ctypes.byref(p), 2, buf, buf, buf, None, buf, buf, buf, None,
                                          None) == EINVAL and want in err()
    if plan is not None:
        assert L.qldpc_extract_key_device(g.handle, ph, 0, 2, buf, buf, None) == EINVAL and want in err()
        # a missing fill is a NULL buffer (the plan punctures 5 positions) ...
        assert L.qldpc_syndrome_batch_device(g.handle, ph, 0, 2, buf, None, None, buf, None) == EINVAL
        assert b"NULL device buffer" in err()
        # ... but not when the plan punctures nothing
        empty = g.rate_plan([], SHORT)
        assert L.qldpc_syndrome_batch_device(g.handle, empty.handle, 0, 2, buf, None, None, buf, None) == EINVAL
        assert b"rate plan does not live" in err()
