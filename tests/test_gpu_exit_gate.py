"""GPU parity of the SPA register decoder's exit gate.

Before the check-node scan of an iteration the kernel may run a parity-only
pass and leave at once when the syndrome is met; at the iteration cap the pass
replaces the check-only scan.  Whether the pass runs is a matter of speed
alone: every case here decodes with QLDPC_EXIT_GATE=-1 (never), with the
largest value (before every checked scan) and with the library's default, and
each must equal the CPU oracle bitwise: hard bits, iteration counts,
syndromes_match and posteriors.  The oracle's result of a case is computed
once and shared by the three runs.
"""
import sys

import numpy as np
import pytest

import qkd_ldpc_v_amd as Q
import shape_codes as S
import test_gpu_parity as GP
import test_gpu_shapes as GS
from conftest import bits_equal_nan, load_fixture
from oracle.pyoracle import Oracle
from test_shape_plans import matrix

pytestmark = pytest.mark.gpu

DBL_MAX = sys.float_info.max
C1, C2 = "c1_n1024_m220.alist", "c2_n10240_m2201.alist"
GATES = {"never": "-1", "always": str(2**31 - 1), "default": None}
_refs, _oracles = {}, {}


@pytest.fixture(params=list(GATES))
def gate(request, monkeypatch):
    """QLDPC_EXIT_GATE is read per launch, under the diagnostic switch."""
    monkeypatch.delenv("QLDPC_EXIT_GATE", raising=False)
    if GATES[request.param] is not None:
        monkeypatch.setenv("QLDPC_DIAG", "1")
        monkeypatch.setenv("QLDPC_EXIT_GATE", GATES[request.param])
    return request.param


def source(name):
    """(H, device graph) of a fixture or of a tests/shape_codes.py case."""
    if name in S.PLANS:
        return matrix(name), GS.graph(name)
    return load_fixture(name), GP.graph(name)


def reference(key, H, max_it, thr_on, llr, synd):
    if key not in _refs:
        if id(H) not in _oracles:
            _oracles[id(H)] = Oracle(H)
        O = _oracles[id(H)]
        _refs[key] = O.decode_batch(O.params(Q.SPA, max_it, thr_on, 100.0), llr, synd, threads=16, posterior=True)
    return _refs[key]


def check(key, name, llr, synd, max_it=50, thr_on=True):
    H, g = source(name)
    ob, oi, ok, op = reference((key, name, max_it, thr_on), H, max_it, thr_on, llr, synd)
    out = g.decode(Q.Params(Q.SPA, max_it, thr_on, 100.0), llr, synd, posterior=True)
    bad = [f for f in range(llr.shape[0])
           if not (np.array_equal(out.bits[f], ob[f]) and out.iterations[f] == oi[f] and out.synd_ok[f] == ok[f]
                   and bits_equal_nan(out.posterior[f], op[f]))]
    assert not bad, (f"{name} cap={max_it}: {len(bad)}/{llr.shape[0]} frames differ; first {bad[0]}: gpu "
                     f"it={out.iterations[bad[0]]} ok={out.synd_ok[bad[0]]} / oracle it={oi[bad[0]]} ok={ok[bad[0]]}")
    return out, (ob, oi, ok, op)


@pytest.mark.parametrize("max_it", [1, 2, 3, 50])
def test_c1_converging_and_failing_frames(gpu_available, gate, max_it):
    """256 frames of C1 at QBER 1.7 %: exits spread over many iterations, and a
    few frames reach the cap."""
    _, _, llr, synd = GP.frames(load_fixture(C1), 0.017, 256, 11)
    _, (_, oi, ok, _) = check("bsc", C1, llr, synd, max_it=max_it)
    if max_it == 50:
        assert 2 <= int((ok == 0).sum()) <= 64 and len(set(oi[ok != 0].tolist())) >= 6


@pytest.mark.parametrize("name", [C1, C2])
def test_frame_that_converges_exactly_at_the_cap(gpu_available, gate, name):
    """One frame whose oracle iteration count is k: at max_iterations = k it
    converges at the cap (the cap's pass finds the syndrome met), at k - 1 it
    fails there."""
    H = load_fixture(name)
    _, _, llr, synd = GP.frames(H, 0.0215 if name == C2 else 0.017, 1, 5)
    _, (_, oi, ok, _) = check("one", name, llr, synd)
    k = int(oi[0])
    assert ok[0] == 1 and 3 <= k < 50
    out, _ = check("one", name, llr, synd, max_it=k)
    assert out.synd_ok[0] == 1 and out.iterations[0] == k
    out, _ = check("one", name, llr, synd, max_it=k - 1)
    assert out.synd_ok[0] == 0 and out.iterations[0] == k - 1


def test_clean_frame(gpu_available, gate):
    """Bob == Alice in frame 0: the channel decision meets the syndrome, and
    the frame leaves where the reference does; its neighbours decode as usual."""
    H = load_fixture(C1)
    a, _, llr, synd = GP.frames(H, 0.017, 4, 3)
    llr[0] = np.abs(llr[0]) * np.where(a[0] != 0, -1.0, 1.0)
    for max_it in (50, 1):
        out, (_, oi, ok, _) = check("clean", C1, llr, synd, max_it=max_it)
        assert ok[0] == 1 and oi[0] <= 1 and out.iterations[0] == oi[0]


@pytest.mark.parametrize("case", ["c1_w3", "degree300_bit", "reg44", "c2_w12"])
def test_register_shapes(gpu_available, gate, case):
    """The SPA register shapes: 40 slots on 3 and on 5 waves, 44 x 16 and
    56 x 12 — rows split across two lanes and lanes that start several rows."""
    H = matrix(case)
    q = 0.03 if case == "degree300_bit" else GS.qber(case, Q.SPA)
    _, _, llr, synd = GP.frames(H, q, 12, 1)
    check("bsc", case, llr, synd)
    check("bsc", case, llr, synd, max_it=2)
    S.assert_plan(GS.graph(case), case, Q.SPA)


@pytest.mark.parametrize("name", [C1, "reg44"])
def test_frames_without_a_palette(gpu_available, gate, name):
    """More than four distinct LLRs per frame (the general iteration-0 scan),
    with +-0, 1e-4 and DBL_MAX in half the frames, NaN and +-inf in others."""
    H, _ = source(name)
    _, _, llr, synd = GP.frames(H, 0.017 if name == C1 else 0.021, 8, 4)
    llr = llr * np.random.default_rng(5).uniform(0.6, 1.4, llr.shape)
    llr[::2, :5] = [1e-4, -1e-4, 0.0, -0.0, DBL_MAX]
    llr[1, 5] = np.nan
    llr[3, [7, 9]] = [np.inf, -np.inf]
    llr[5, [11, 12, 13]] = [np.nan, np.inf, -np.inf]
    check("soft", name, llr, synd)
    check("soft", name, llr, synd, max_it=3, thr_on=False)


def test_c2_bench_operating_point(gpu_available, gate):
    """64 frames of C2 at QBER 2.15 %: the 40 x 16 shape with message slots in
    LDS that the benchmark runs."""
    _, _, llr, synd = GP.frames(load_fixture(C2), 0.0215, 64, 7)
    _, (_, oi, ok, _) = check("bsc", C2, llr, synd)
    assert int((ok != 0).sum()) >= 32 and len(set(oi.tolist())) >= 4
