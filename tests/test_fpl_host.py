"""The frame-per-lane layout on host-only graphs: qldpc_graph_create_opts'
validation, what an `fpl` graph reports, AUTO through the new entry against
the existing entries, the paired-adjacency refusal and the diagnostic knob.
No device is touched."""
import ctypes
import os

import numpy as np
import pytest

import qkd_ldpc_v_amd as Q
import shape_codes as S
from conftest import diag_env, load_fixture
from qkd_ldpc_v_amd import _lib

C1 = "c1_n1024_m220.alist"
EINVAL, EUNSUP = -1, -5


def create_opts(H, opts, bit_nodes=True):
    """qldpc_graph_create_opts on H, no device list -> (rc, handle)."""
    g = ctypes.c_void_p()
    rc = Q.lib().qldpc_graph_create_opts(H.n, H.m, _lib.ptr(H.row_ptr), _lib.ptr(H.col_idx),
                                         _lib.ptr(H.col_ptr) if bit_nodes else None,
                                         _lib.ptr(H.row_idx) if bit_nodes else None, None, 0,
                                         None if opts is None else ctypes.byref(opts), ctypes.byref(g))
    return rc, g


def host_opts(layout=_lib.LAYOUT_AUTO):
    return _lib.qldpc_graph_opts(layout, 1)


def test_unknown_layout_and_reserved_words_are_refused():
    H = load_fixture(C1)
    for layout in (2, -1, 1 << 20):
        rc, g = create_opts(H, host_opts(layout))
        assert rc == EINVAL and not g.value, layout
        assert b"layout" in Q.lib().qldpc_last_error()
    for word in range(6):
        o = host_opts(_lib.LAYOUT_FRAME_PER_LANE)
        o.reserved[word] = 1
        rc, g = create_opts(H, o)
        assert rc == EINVAL and not g.value, word
        assert b"reserved" in Q.lib().qldpc_last_error()
    with pytest.raises(ValueError):
        Q.Graph(H, host_only=True, layout="frame_major")


@pytest.mark.parametrize("case", ["c1", "split_k4", "long_row41", "empty_row_first", "degree510_bit"])
def test_fpl_graph_reports_its_plan(case):
    H = load_fixture(C1) if case == "c1" else S.CODES[case]()
    g = Q.Graph(H, host_only=True, layout="frame_per_lane")
    for alg in range(6):
        assert g.plan(0, alg) == {"lanes": 64, "edges_per_lane": 0, "workgroups": None, "lds_bytes": 0,
                                  "variant": "fpl"}
    assert g.split_plan() == {"parts": 1, "part_lanes": 64, "scratch_slots": 0}
    lab, _ = g.labels()
    assert np.array_equal(lab, np.arange(H.n))
    assert g.info() == {"n": H.n, "m": H.m, "nnz": H.nnz, "devices": 0}


def test_fpl_takes_an_empty_row_between_two_others():
    """The register layouts refuse it (a lane's row counter); fpl walks row_ptr."""
    H = S.empty_row(200)
    with pytest.raises(Q.QLDPCError):
        Q.Graph(H, host_only=True)
    assert Q.Graph(H, host_only=True, layout="frame_per_lane").plan()["variant"] == "fpl"


@pytest.mark.parametrize("case", ["c1", "split_k4", "long_row41", "empty_row_first"])
def test_auto_through_the_new_entry_is_the_existing_graph(case):
    H = load_fixture(C1) if case == "c1" else S.CODES[case]()
    want = Q.Graph(H, host_only=True)
    assert want.plan()["variant"] != "fpl"
    for bit_nodes in (True, False):  # (bit_nodes absent: their ascending transpose)
        rc, h = create_opts(H, host_opts(), bit_nodes)
        assert rc == 0, Q.lib().qldpc_last_error()
        g = Q.Graph.__new__(Q.Graph)
        g.H, g.n, g.m, g.host_only, g._g = H, H.n, H.m, True, h
        for alg in range(6):
            assert g.plan(0, alg) == want.plan(0, alg), (case, alg)
        assert g.split_plan() == want.split_plan()
        la, sa = g.labels()
        lb, sb = want.labels()
        assert np.array_equal(la, lb) and sa == sb


def test_paired_adjacency_is_refused_for_fpl():
    """c1's bit_nodes with one bit's check list reversed: the reference's
    occurrence pairing is no longer the edge itself."""
    H = load_fixture(C1)
    i = int(np.argmax(np.diff(H.col_ptr) >= 2))
    ri = H.row_idx.copy()
    ri[H.col_ptr[i]:H.col_ptr[i + 1]] = ri[H.col_ptr[i]:H.col_ptr[i + 1]][::-1]
    Hp = Q.HMatrix(H.n, H.m, H.row_ptr, H.col_idx, H.col_ptr, ri)
    with pytest.raises(Q.QLDPCError) as e:
        Q.Graph(Hp, host_only=True, layout="frame_per_lane")
    assert e.value.code == EUNSUP and "occurrence pairing" in str(e.value)
    rc, h = create_opts(Hp, host_opts())  # AUTO still plans it (v1)
    assert rc == 0
    Q.lib().qldpc_graph_destroy(h)


def test_variant_knob_needs_the_diagnostic_switch(monkeypatch):
    H = load_fixture(C1)
    monkeypatch.delenv("QLDPC_DIAG", raising=False)
    monkeypatch.setenv("QLDPC_VARIANT", "fpl")
    assert Q.Graph(H, host_only=True).plan()["variant"] == "v2"
    monkeypatch.delenv("QLDPC_VARIANT")
    with diag_env(QLDPC_VARIANT="fpl"):
        g = Q.Graph(H, host_only=True)
    assert "QLDPC_VARIANT" not in os.environ
    assert g.plan()["variant"] == "fpl" and g.split_plan()["part_lanes"] == 64


def test_new_symbol_is_bound():
    assert "qldpc_graph_create_opts" in _lib.exported_symbols()
