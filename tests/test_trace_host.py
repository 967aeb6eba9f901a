"""The per-iteration trace entries on host-only graphs: the symbols are bound,
and the argument checks that come before any device is touched answer in their
documented order (NULL graph, parameters, batch < 0, layout, batch == 0)."""
import ctypes
import math

import numpy as np
import pytest

import qkd_ldpc_v_amd as Q
from conftest import load_fixture
from qkd_ldpc_v_amd import _lib

C1 = "c1_n1024_m220.alist"
EINVAL = -1


def empty(H):
    return np.empty((0, H.n)), np.empty((0, H.m), np.uint8)


def test_trace_symbols_are_bound():
    assert {"qldpc_decode_trace_batch", "qldpc_decode_trace_batch_device"} <= set(_lib.exported_symbols())
    assert Q.TRACE_NONE == 0xFFFFFFFF


def test_other_layouts_are_refused_before_the_batch_is_looked_at():
    H = load_fixture(C1)
    g = Q.Graph(H, host_only=True)
    assert g.plan()["variant"] != "fpl"
    with pytest.raises(Q.QLDPCError, match="EUNSUP.*frame_per_lane") as e:
        g.decode_trace(Q.Params(Q.SPA, 50), *empty(H))
    assert e.value.code == -5
    p = Q.Params(Q.SPA, 50).c()
    rc = Q.lib().qldpc_decode_trace_batch_device(g.handle, 0, ctypes.byref(p), 0, None, None, None, None, None, None,
                                                 None, None, None)
    assert rc == -5 and b"frame_per_lane" in Q.lib().qldpc_last_error()


def test_empty_batch_on_a_frame_per_lane_graph():
    H = load_fixture(C1)
    g = Q.Graph(H, host_only=True, layout="frame_per_lane")
    out = g.decode_trace(Q.Params(Q.AOMSA, 7, True, 100.0, 0.55, 1.2), *empty(H), posterior=True, trace_posterior=True)
    assert out.bits.shape == (0, H.n) and out.iterations.shape == (0,) and out.synd_ok.shape == (0,)
    assert out.posterior.shape == (0, H.n)
    assert out.unsat.shape == (0, 7) and out.unsat.dtype == np.uint32
    assert out.trace_posterior.shape == (0, 7, H.n) and out.rows.shape == (0,)
    assert g.decode_trace(Q.Params(Q.SPA, 7), *empty(H)).trace_posterior is None
    p = Q.Params(Q.SPA, 7).c()
    assert Q.lib().qldpc_decode_trace_batch_device(g.handle, 0, ctypes.byref(p), 0, None, None, None, None, None, None,
                                                   None, None, None) == 0


def test_parameters_and_batch_are_checked_before_the_layout():
    H = load_fixture(C1)
    auto = Q.Graph(H, host_only=True)
    for thr in (0.0, -1.0, math.nan):
        with pytest.raises(Q.QLDPCError, match="EINVAL.*threshold must be > 0"):
            auto.decode_trace(Q.Params(Q.SPA, 50, True, thr), *empty(H))
    p = Q.Params(Q.SPA, 50).c()
    L = Q.lib()
    assert L.qldpc_decode_trace_batch(auto.handle, ctypes.byref(p), -1, None, None, None, None, None, None, None,
                                      None) == EINVAL
    assert b"batch" in L.qldpc_last_error()
    assert L.qldpc_decode_trace_batch(None, ctypes.byref(p), 0, None, None, None, None, None, None, None,
                                      None) == EINVAL
    assert b"graph is NULL" in L.qldpc_last_error()
