"""The launch shape of every (graph, algorithm), pinned on the CPU (no GPU).

Which decode_v2_kernel instantiation decodes a graph, with how many threads
and how much LDS, is decided once per call (plan.hip launch_shape, decoder_v2.hip
v2_launch_shape).  Under QLDPC_DIAG=1 with QLDPC_DEBUG_PLAN the library prints
one `{"launch": {...}}` line per algorithm 0..5 when a graph is created: the
shape's fields and its name, e.g. v2<alg=0,R=40,RG=0,RL=5,split=1,pl=1024,vng=0,rglb=0>.

tests/golden/launch_shapes.json was recorded from the commit before the launch
shape existed, not from the code under test: a throw-away print in that
commit's build_graph evaluated its own lds_of and block_threads, its
decode_on predicates for the bit gather (VNG) and the rows in global scratch
(RGLB), v2_use_rl / v2_use_rl_split on the arguments decode_on would fill, and
the template arguments its launch_decode_v2 / kernel_v2 / kernel_v2_vng /
kernel_split would select for them, and wrote them in this line's format.
(rows_lds is the row count that commit's lds_of gave V2Layout; on v1 and
frame-per-lane graphs the V2 fields are 0 / their defaults.)

A later intentional change of a shape re-records the file (run with -s: each
case prints its lines before it asserts).
"""
import ctypes
import json
import os

import pytest

import shape_codes as S
from conftest import GOLDEN, diag_env, load_fixture
from qkd_ldpc_v_amd._lib import lib, ptr
from test_layout import CASES as LAYOUT_CASES
from test_shape_plans import matrix as shape_matrix

SHAPE_CASES = ["reg44", "c2_w12", "c1_w2", "hybrid_dv4_lds", "hybrid_dv4_global", "split_k4", "split_k2_w8",
               "split_k2_w16", "long_row33", "degree510_bit"]

# id -> (matrix, knobs under QLDPC_DIAG=1)
CASES = {case: (make, knobs) for case, (make, knobs, _) in LAYOUT_CASES.items()}
CASES.update({case: ((lambda case=case: shape_matrix(case)), S.KNOBS.get(case, {})) for case in SHAPE_CASES})
# QLDPC_VNG=0: VN phases instead of the min-sum bit gather (read when the line is printed, as at every launch)
for _case in ("c3", "c5", "hybrid_dv4_lds"):
    CASES[_case + "_vng0"] = (CASES[_case][0], dict(CASES[_case][1], QLDPC_VNG="0"))
CASES["c1_fpl"] = (CASES["c1"][0], {"QLDPC_VARIANT": "fpl"})  # the frame-per-lane layout prints its lines too


def launch_lines(H, knobs):
    """The six launch lines of a host-only graph of H, and qldpc_graph_plan's answer per algorithm."""
    g = ctypes.c_void_p()
    with diag_env(QLDPC_DEBUG_PLAN="1", **knobs):
        rc = lib().qldpc_graph_create_host(H.n, H.m, ptr(H.row_ptr), ptr(H.col_idx), ctypes.byref(g))
        assert rc == 0, rc
        plans = []
        for alg in range(6):
            lanes, epl, lds = (ctypes.c_int32() for _ in range(3))
            var = ctypes.c_char_p()
            rc = lib().qldpc_graph_plan(g, 0, alg, ctypes.byref(lanes), ctypes.byref(epl), None, ctypes.byref(lds),
                                        ctypes.byref(var))
            assert rc == 0, rc
            plans.append({"lanes": lanes.value, "lds_bytes": lds.value, "variant": var.value.decode()})
        lib().qldpc_graph_destroy(g)
    return plans


def _parse(err):
    return [json.loads(line)["launch"] for line in err.splitlines() if line.startswith('{"launch"')]


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(GOLDEN, "launch_shapes.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("case", list(CASES))
def test_launch_lines_match_the_recorded_shapes(case, recorded, capfd, monkeypatch):
    make, knobs = CASES[case]
    H = make()
    monkeypatch.delenv("QLDPC_DIAG", raising=False)
    monkeypatch.delenv("QLDPC_DEBUG_PLAN", raising=False)
    monkeypatch.delenv("QLDPC_VNG", raising=False)
    capfd.readouterr()
    plans = launch_lines(H, knobs)
    got = _parse(capfd.readouterr().err)
    for line in got:
        print(f"launch {case}: {json.dumps(line)}")
    want = recorded[case]
    assert len(want) == 6 and [w["alg"] for w in want] == list(range(6))
    assert len(got) == 6, got
    for g, w, plan in zip(got, want, plans):
        assert g == w, (case, g, w)
        assert plan == {k: g[k] for k in ("lanes", "lds_bytes", "variant")}, (case, plan, g)


def test_the_cases_reach_every_kind_of_shape(recorded):
    """What the table is for: LDS message slots on one-workgroup and split
    frames, the bit gather on both of its shapes and with rows in global
    scratch, every register shape, both part sizes, v1 and frame-per-lane."""
    names = {line["name"] for lines in recorded.values() for line in lines}
    for part in ("R=40,RG=0,RL=5,split=1", "R=44,RG=0,RL=0", "R=56,RG=0,RL=0", "R=44,RG=20,RL=0,split=1,pl=1024,vng=0",
                 "R=40,RG=0,RL=0,split=1,pl=1024,vng=1,rglb=0", "R=44,RG=20,RL=0,split=1,pl=1024,vng=1,rglb=0",
                 "R=44,RG=20,RL=0,split=1,pl=1024,vng=1,rglb=1", "pl=512,vng=0", "RG=12,RL=16,split=2,pl=1024",
                 "RG=12,RL=12,split=2,pl=512", "reg_lds<", "glb_lds<", "glb_glb<", "fpl<"):
        assert any(part in n for n in names), part
    # QLDPC_VNG=0 moves the min-sum algorithms off the bit gather and nothing else
    for case in ("c3", "c5", "hybrid_dv4_lds"):
        on, off = recorded[case], recorded[case + "_vng0"]
        assert [line["vng"] for line in on] == [0, 0, 1, 1, 1, 1] and not any(line["vng"] for line in off)
        strip = lambda line: {k: v for k, v in line.items() if k not in ("vng", "name")}
        assert [strip(a) for a in on] == [strip(b) for b in off]


def test_launch_lines_need_the_diag_switch(capfd, monkeypatch):
    monkeypatch.delenv("QLDPC_DIAG", raising=False)
    monkeypatch.setenv("QLDPC_DEBUG_PLAN", "1")
    capfd.readouterr()
    H = load_fixture("c1_n1024_m220.alist")
    g = ctypes.c_void_p()
    assert lib().qldpc_graph_create_host(H.n, H.m, ptr(H.row_ptr), ptr(H.col_idx), ctypes.byref(g)) == 0
    lib().qldpc_graph_destroy(g)
    assert "launch" not in capfd.readouterr().err
