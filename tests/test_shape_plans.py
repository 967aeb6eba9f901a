"""The plans of the generated shape codes, pinned on the CPU (no GPU).

tests/test_gpu_shapes.py decodes tests/shape_codes.py's codes because each
reaches a kernel instantiation, layout branch or row structure that no
committed matrix plans.  A planner change could quietly move one of them onto
a shape that is already covered; this file pins what the host planner does
with each (shape_codes.PLANS), from Graph.plan(), Graph.split_plan() and the
`{"plan": ...}` line the library prints under QLDPC_DIAG=1 with
QLDPC_DEBUG_PLAN (V2 plans only; run with -s to see each line).

Empty check rows: before the first and after the last non-empty row they are
decoded (v1); anywhere between two non-empty rows the graph is refused.
"""
import json

import pytest

import qkd_ldpc_v_amd as Q
import shape_codes as S
from conftest import diag_env, load_fixture
from qkd_ldpc_v_amd._lib import QLDPCError

FIXTURES = {"c2_w12": "c2_n10240_m2201.alist", "c1_w2": "c1_n1024_m220.alist", "c1_w3": "c1_n1024_m220.alist"}
REFUSAL = "empty check rows between non-empty rows are not supported"


def matrix(case):
    return load_fixture(FIXTURES[case]) if case in FIXTURES else S.CODES[case]()


@pytest.mark.parametrize("case", list(S.PLANS))
def test_case_reaches_its_plan(case, capfd, monkeypatch):
    H = matrix(case)
    monkeypatch.delenv("QLDPC_DIAG", raising=False)
    monkeypatch.delenv("QLDPC_DEBUG_PLAN", raising=False)
    capfd.readouterr()
    with diag_env(QLDPC_DEBUG_PLAN="1", **S.KNOBS.get(case, {})):
        g = Q.Graph(H, host_only=True)
    lines = [json.loads(line)["plan"] for line in capfd.readouterr().err.splitlines() if line.startswith('{"plan"')]
    print(f"plan {case}: {g.plan()} {g.split_plan()} {lines}")
    want = S.PLANS[case]
    S.assert_plan(g, case)
    if want["debug"] is None:  # v1: the line is V2's
        assert lines == []
    else:
        assert len(lines) == 1, lines
        assert {k: lines[0][k] for k in want["debug"]} == want["debug"], (case, lines[0])
        assert lines[0]["epl_max"] == want["edges_per_lane"]
        if case.startswith("hybrid_dv4"):  # layout.hip vn_stage(): no high-degree stage on this hybrid shape
            assert lines[0]["dv_max"] == 4


def test_cases_cover_the_shapes_they_were_written_for():
    """What the GPU tests rely on, said once: the PLANS table itself holds the
    44- and 56-slot register shapes, the hybrid shape, rows partly in global
    scratch, K = 2 (both part sizes), 3 and 4 split frames, an odd wave count
    and the v1 fallbacks reg_lds and glb_lds."""
    P = S.PLANS
    assert P["reg44"]["debug"]["slots_reg"] == 44 and P["reg44_full"]["edges_per_lane"] == 44
    assert P["c2_w12"]["debug"]["slots_reg"] == 56 and P["c2_w12"]["lanes"] == 768
    assert P["hybrid_dv4_lds"]["debug"]["slots_scratch"] == 20 and not P["hybrid_dv4_lds"]["debug"]["rows_global_ms"]
    assert P["hybrid_dv4_global"]["debug"]["rows_global_ms"] == 1
    assert [P[c]["split"]["parts"] for c in ("split_k2_w8", "split_k2_w16", "split_k4_isolated", "split_k4")] == \
        [2, 2, 3, 4]
    assert P["split_k2_w8"]["split"]["part_lanes"] == 512 and P["split_k2_w16"]["split"]["part_lanes"] == 1024
    # test_gpu_long_frames.py: split frames of an odd n at which the per-frame kernels launch 1024 threads
    H = S.long_split()
    assert P["long_split"]["split"]["parts"] == 2 and H.n >= 32768 and H.n % 2 == 1
    assert P["long_row32"]["debug"]["waves"] == 3
    assert [P[f"long_row{d}"]["variant"] for d in (33, 40, 41)] == ["reg_lds", "reg_lds", "glb_lds"]


def _created(H):
    try:
        Q.Graph(H, host_only=True).close()
        return None
    except QLDPCError as e:
        return e


def test_one_empty_row_at_every_position():
    """The 2000 x 400 code with one empty check inserted before row `at`, for
    every at in 0..m: accepted at 0 and m only, refused with EUNSUP and the
    one message everywhere else — also where the row falls on a lane boundary
    of the v1 layout (the lane loop used to miss it there)."""
    m = S.base_2000x400().m
    accepted, other = [], []
    for at in range(m + 1):
        e = _created(S.with_rows(S.base_2000x400(), [[]], at=at))
        if e is None:
            accepted.append(at)
        elif not (e.code == -5 and REFUSAL in str(e)):
            other.append((at, str(e)))
    assert accepted == [0, m], accepted
    assert not other, other[:3]


@pytest.mark.parametrize("at", [1, 61, 200, 399])
def test_two_adjacent_empty_rows_in_the_middle(at):
    e = _created(S.with_rows(S.base_2000x400(), [[], []], at=at))
    assert e is not None and e.code == -5 and REFUSAL in str(e), e


def test_empty_rows_at_both_ends_together():
    H = S.with_rows(S.with_rows(S.base_2000x400(), [[], []], at=0), [[]])
    assert _created(H) is None
    assert Q.Graph(H, host_only=True).plan()["variant"] == "reg_lds"
