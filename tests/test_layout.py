"""The planner's index tables, pinned by a digest (host only, no GPU).

layout.hip turns H into about 35 index tables (slot metadata, VN masks, the
bit-gather and exchange layouts, row-ELL ...).  A wrong table gives wrong bits
or a part group that never meets, and nothing else on the CPU sees their
contents.  Under QLDPC_DIAG=1 with QLDPC_DEBUG_PLAN the library prints
`{"layout": {"digest": ...}}`: 64-bit FNV-1a over the plan's scalars and every
table (layout_digest).  The values below were recorded from the commit before
the tables' code was split out of capi.hip, with the same digest function
applied to its build_graph locals — not from the code under test.

A later intentional layout change re-records these values (run this file with
-s: each case prints its digest before it asserts).
"""
import ctypes
import json

import pytest

import qkd_ldpc_v_amd as Q
from conftest import diag_env, load_fixture
from qkd_ldpc_v_amd._lib import lib, ptr
from test_unsorted import permuted


def _fixture(name):
    return lambda: load_fixture(name)


C1, C2, C3 = "c1_n1024_m220.alist", "c2_n10240_m2201.alist", "c3_n10240_m1801.alist"
C5, C5B, C5C = "c5_n10240_m2048.sp2", "c5b_n10240_m3584.sp2", "c5c_n10240_m5120.sp2"
C4S = "c4s_n102400_m32001.alist"

# id -> (matrix, knobs under QLDPC_DIAG=1, digest of the parent's tables)
CASES = {
    "kat": (_fixture("kat_n6_m4.dense"), {}, "540d9f4898da1bd0"),
    "c1": (_fixture(C1), {}, "f316a916976daee8"),
    "c2": (_fixture(C2), {}, "7bf9e5dfab18ac7a"),
    "c3": (_fixture(C3), {}, "68f28b8392fe86ae"),
    "c5": (_fixture(C5), {}, "8e8ae367e306b112"),
    "c5b": (_fixture(C5B), {}, "a22f1adca3638f7b"),
    "c5c": (_fixture(C5C), {}, "5215ef25e4ad3456"),
    "c4s": (_fixture(C4S), {}, "ae95eb0990eabab4"),
    "c4ii": (lambda: Q.regular_code(102400, 22001, 4, 777), {}, "0fd35d5080c50af9"),
    # the three v1 layouts: reg_lds, glb_lds, glb_glb
    "c1_v1": (_fixture(C1), {"QLDPC_VARIANT": "v1"}, "e008c83fa88e662b"),
    "c5_v1": (_fixture(C5), {"QLDPC_VARIANT": "v1"}, "5c48eea4235ebd31"),
    "c4s_v1": (_fixture(C4S), {"QLDPC_VARIANT": "v1"}, "28b16db160af4518"),
    "c4s_x0": (_fixture(C4S), {"QLDPC_SPLIT_X": "0"}, "0d5c3b9f19aa560a"),
    "c4s_k10": (_fixture(C4S), {"QLDPC_SPLIT_K": "10"}, "c6b20b6bd6f1e316"),
    "c2_norelabel": (_fixture(C2), {"QLDPC_RELABEL": "0"}, "de3157f0f933fcbc"),
    # unsorted check_nodes rows: occurrence pairing (tests/test_unsorted.py)
    "c1_unsorted": (lambda: permuted(load_fixture(C1), 1, rows=True, cols=False), {}, "eb901730cdb6fbd6"),
}


def _host_graph(H):
    g = ctypes.c_void_p()
    rc = lib().qldpc_graph_create_host(H.n, H.m, ptr(H.row_ptr), ptr(H.col_idx), ctypes.byref(g))
    assert rc == 0, rc
    lib().qldpc_graph_destroy(g)


def _layout_lines(err):
    return [json.loads(line)["layout"]["digest"] for line in err.splitlines() if line.startswith('{"layout"')]


@pytest.mark.parametrize("case", list(CASES))
def test_layout_digest_matches_the_recorded_tables(case, capfd, monkeypatch):
    make, knobs, want = CASES[case]
    H = make()
    monkeypatch.delenv("QLDPC_DIAG", raising=False)
    monkeypatch.delenv("QLDPC_DEBUG_PLAN", raising=False)
    capfd.readouterr()
    with diag_env(QLDPC_DEBUG_PLAN="1", **knobs):
        _host_graph(H)
    got = _layout_lines(capfd.readouterr().err)
    print(f"layout digest {case}: {got}")
    assert len(got) == 1 and len(got[0]) == 16, got
    assert got[0] == want, (case, got[0], want)


def test_layout_line_needs_the_diag_switch(capfd, monkeypatch):
    monkeypatch.delenv("QLDPC_DIAG", raising=False)
    monkeypatch.setenv("QLDPC_DEBUG_PLAN", "1")
    capfd.readouterr()
    _host_graph(load_fixture(C1))
    assert "layout" not in capfd.readouterr().err
