"""GPU parity of the per-iteration decode trace (Graph.decode_trace on a
frame-per-lane graph, decoder_fpl.hip) against the CPU oracle's
Oracle.decode(..., trace=True) — never against another GPU run.

Row `it` of a frame exists when the bit pass of iteration `it` ran for it:
iterations_num rows for SPA / SPA-LIN / NMSA / OMSA; for ANMSA / AOMSA, which
leave after a check-node pass, iterations_num - 1 rows on a match and
max_iterations rows otherwise.  The expected count of a row is the number of
checks whose parity over the oracle's decisions (total <= 0) misses the
syndrome bit, as tools/exit_gate_stats.py forms it (H.syndrome also takes
empty rows).  Written posterior rows are compared bitwise, rows that do not
exist must read TRACE_NONE / the all-ones NaN, and the plain outputs are the
plain decode's.
"""
import sys

import numpy as np
import pytest

import qkd_ldpc_v_amd as Q
import shape_codes as S
from conftest import bits_equal_nan, diag_env, load_fixture
from oracle.pyoracle import Oracle
from test_gpu_fpl import _graphs, _oracles, graph, matrix, oracle
from test_gpu_parity import ALGS, frames
from test_gpu_shapes import QBER as SHAPE_QBER

pytestmark = pytest.mark.gpu

DBL_MAX = sys.float_info.max
C1, C2 = "c1_n1024_m220.alist", "c2_n10240_m2201.alist"
SPA, OMSA, ANMSA, AOMSA = ALGS[0], ALGS[3], ALGS[4], ALGS[5]
ALL_ONES = np.uint64(0xFFFFFFFFFFFFFFFF)
_built = {}  # matrices a test builds itself, by the name of their graph


def expected_rows(alg, it, ok, max_it):
    if alg in (Q.ANMSA, Q.AOMSA):
        return it - 1 if ok else max_it
    return it


def oracle_trace(name, alg, prim, sec, llr, synd, max_it=50, thr_on=True, post_frames=None):
    """The oracle's plain outputs, row counts, unsat[batch, max_it] and the
    posterior rows of the first post_frames frames (None: all)."""
    H, O = _built.get(name) or matrix(name), oracle(name)
    p = O.params(alg, max_it, thr_on, 100.0, prim, sec)
    B = llr.shape[0]
    npost = B if post_frames is None else post_frames
    bits = np.empty((B, H.n), np.uint8)
    iters, oks, rows = np.empty(B, np.uint32), np.empty(B, np.uint8), np.empty(B, np.int64)
    post = np.empty((B, H.n))
    unsat = np.full((B, max_it), Q.TRACE_NONE, np.uint32)
    tpost = np.full((npost, max_it, H.n), np.nan)
    for f in range(B):
        bits[f], it, ok, post[f], tr = O.decode(p, llr[f], synd[f], trace=True)
        iters[f], oks[f] = it, ok
        r = rows[f] = expected_rows(alg, it, ok, max_it)
        if r > 0:
            z = (tr[:r] <= 0.0).astype(np.uint8)
            unsat[f, :r] = (H.syndrome(z) != synd[f][None, :]).sum(axis=1)
        if f < npost:
            tpost[f, :r] = tr[:r]
    return bits, iters, oks, post, rows, unsat, tpost


def assert_trace(out, ref, what):
    bits, iters, oks, post, rows, unsat, tpost = ref
    assert np.array_equal(out.bits, bits) and np.array_equal(out.iterations, iters), what
    assert np.array_equal(out.synd_ok, oks), what
    if out.posterior is not None:
        assert bits_equal_nan(out.posterior, post), what
    assert np.array_equal(out.rows, rows), (what, out.rows.tolist(), rows.tolist())
    bad = np.argwhere(out.unsat != unsat)
    assert bad.size == 0, f"{what}: unsat differs at (frame, row) {bad[:5].tolist()}"
    if out.trace_posterior is not None:
        for f in range(out.trace_posterior.shape[0]):
            r = int(rows[f])
            assert bits_equal_nan(out.trace_posterior[f, :r], tpost[f, :r]), f"{what}: frame {f} posterior rows"
            assert (out.trace_posterior[f, r:].view(np.uint64) == ALL_ONES).all(), f"{what}: frame {f} rows past {r}"


def assert_trace_parity(name, alg, prim, sec, llr, synd, max_it=50, thr_on=True, ref=None):
    out = graph(name).decode_trace(Q.Params(alg, max_it, thr_on, 100.0, prim, sec), llr, synd, posterior=True,
                                   trace_posterior=True)
    if ref is None:
        ref = oracle_trace(name, alg, prim, sec, llr, synd, max_it, thr_on)
    assert_trace(out, ref, f"{name} alg={alg} cap={max_it} thr={thr_on}")
    return out, ref


# ---- 1. two full tiles and a two-lane tail, early and capped lanes in each tile ----------------------
@pytest.mark.parametrize("alg,prim,sec", ALGS)
def test_tiles_and_tail(gpu_available, alg, prim, sec):
    _, _, llr, synd = frames(load_fixture(C1), 0.02, 130, seed=1)
    out, ref = assert_trace_parity(C1, alg, prim, sec, llr, synd)
    if alg == Q.ANMSA:
        # capped, unmatched, and no check off after the last bit pass: the reference never tests those decisions
        quirk = (out.iterations == 50) & (out.synd_ok == 0) & (out.unsat[:, 49] == 0)
        assert quirk.any()
    with diag_env(QLDPC_ORDER="0"):
        assert_trace_parity(C1, alg, prim, sec, llr, synd, ref=ref)
    with diag_env(QLDPC_FPL_TILES="1"):
        assert_trace_parity(C1, alg, prim, sec, llr, synd, ref=ref)


# ---- 2. exit edges ----------------------------------------------------------------------------------
@pytest.mark.parametrize("alg,prim,sec", [SPA, OMSA, AOMSA])
def test_exit_edges(gpu_available, alg, prim, sec):
    H = load_fixture(C1)
    for max_it in (1, 2, 3):
        _, _, llr, synd = frames(H, 0.02, 5, seed=700 + max_it)
        assert_trace_parity(C1, alg, prim, sec, llr, synd, max_it=max_it)
    _, _, llr, synd = frames(H, 1e-6, 5, seed=750)
    out, _ = assert_trace_parity(C1, alg, prim, sec, llr, synd)
    if alg == Q.AOMSA:  # left before the first bit pass
        assert (out.rows == 0).all() and (out.unsat == Q.TRACE_NONE).all()
        assert (out.trace_posterior.view(np.uint64) == ALL_ONES).all()
    else:
        assert (out.rows == 1).all() and (out.unsat[:, 0] == 0).all()


# ---- 3. row structures ------------------------------------------------------------------------------
@pytest.mark.parametrize("alg,prim,sec", [SPA, OMSA, AOMSA])
@pytest.mark.parametrize("case", ["empty_row_first", "long_row41", "degree1_rows"])
def test_row_structures(gpu_available, case, alg, prim, sec):
    q, own = SHAPE_QBER[case]
    _, _, llr, synd = frames(matrix(case), own.get(alg, q), 12, seed=1)
    assert_trace_parity(case, alg, prim, sec, llr, synd)


def test_empty_row_with_its_syndrome_bit_set(gpu_available):
    """An empty check whose syndrome bit is 1 is off in every row of the trace."""
    H = S.empty_row(200)
    name = "empty_row_mid"
    _built[name] = H
    if name not in _graphs:
        _graphs[name] = Q.Graph(H, layout="frame_per_lane")
        _oracles[name] = Oracle(H)
    _, _, llr, synd = frames(H, 0.010, 8, seed=1)
    synd = synd.copy()
    synd[::2, 200] = 1
    for alg, prim, sec in (SPA, OMSA, AOMSA):
        out, _ = assert_trace_parity(name, alg, prim, sec, llr, synd, max_it=12)
        assert (out.rows[::2] == 12).all() and (out.unsat[::2] >= 1).all()


# ---- 4. special LLR values --------------------------------------------------------------------------
@pytest.mark.parametrize("thr_on", [True, False])
@pytest.mark.parametrize("alg,prim,sec", [SPA, AOMSA])
def test_special_llrs(gpu_available, alg, prim, sec, thr_on):
    H = load_fixture(C1)
    _, _, llr, synd = frames(H, 0.02, 16, seed=60 + alg)
    llr = llr * np.random.default_rng(61 + alg).uniform(0.6, 1.4, llr.shape)
    llr[::2, :8] = [1e-4, -1e-4, 0.0, -0.0, DBL_MAX, np.inf, -np.inf, np.nan]
    assert_trace_parity(C1, alg, prim, sec, llr, synd, thr_on=thr_on)


# ---- 5. C2: counts of up to several hundred rows ----------------------------------------------------
@pytest.mark.parametrize("alg,prim,sec", [SPA, AOMSA])
def test_c2_counts(gpu_available, alg, prim, sec):
    _, _, llr, synd = frames(load_fixture(C2), 0.0215, 66, seed=5)
    ref = oracle_trace(C2, alg, prim, sec, llr, synd, post_frames=3)
    p = Q.Params(alg, 50, True, 100.0, prim, sec)
    out = graph(C2).decode_trace(p, llr, synd, posterior=True)
    assert out.trace_posterior is None
    assert_trace(out, ref, f"c2 alg={alg} counts")
    assert (ref[1] == 50).any() and ref[1].min() < 50 and ref[5][ref[5] != Q.TRACE_NONE].max() > 64
    first = graph(C2).decode_trace(p, llr[:3], synd[:3], posterior=True, trace_posterior=True)
    assert_trace(first, tuple(x[:3] for x in ref), f"c2 alg={alg} posterior rows")


# ---- 6. entries -------------------------------------------------------------------------------------
def test_device_entry_on_a_side_stream(gpu_available):
    import torch

    H = load_fixture(C1)
    g = graph(C1)
    alg, prim, sec = OMSA
    p = Q.Params(alg, 50, True, 100.0, prim, sec)
    _, _, llr, synd = frames(H, 0.02, 70, seed=31)
    dev = torch.device("cuda:0")
    st = torch.cuda.Stream(device=dev)
    tl, ts = torch.from_numpy(llr).to(dev), torch.from_numpy(synd).to(dev)
    bits = torch.empty((70, H.n), dtype=torch.uint8, device=dev)
    it = torch.empty(70, dtype=torch.int32, device=dev)
    ok = torch.empty(70, dtype=torch.uint8, device=dev)
    unsat = torch.zeros((70, 50), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    g.decode_trace_device(p, tl, ts, bits, it, ok, None, unsat, None, stream=st)
    st.synchronize()
    out = Q.TraceOutput(bits.cpu().numpy(), it.cpu().numpy().astype(np.uint32), ok.cpu().numpy(), None,
                        unsat.cpu().numpy().view(np.uint32), None)
    assert_trace(out, oracle_trace(C1, alg, prim, sec, llr, synd, post_frames=0), "device entry")
    # both trace pointers NULL: the plain decode
    b2, i2, k2 = torch.zeros_like(bits), torch.zeros_like(it), torch.zeros_like(ok)
    g.decode_trace_device(p, tl, ts, b2, i2, k2, None, None, None, stream=st)
    b3, i3, k3 = torch.zeros_like(bits), torch.zeros_like(it), torch.zeros_like(ok)
    g.decode_device(p, tl, ts, b3, i3, k3, None, stream=st)
    st.synchronize()
    assert torch.equal(b2, b3) and torch.equal(i2, i3) and torch.equal(k2, k3)
    assert torch.equal(b2, bits) and torch.equal(i2, it)


def test_two_shards_on_one_device(gpu_available):
    H = load_fixture(C1)
    g = Q.Graph(H, devices=[0, 0], layout="frame_per_lane")
    alg, prim, sec = AOMSA
    _, _, llr, synd = frames(H, 0.02, 130, seed=33)
    out = g.decode_trace(Q.Params(alg, 50, True, 100.0, prim, sec), llr, synd, posterior=True, trace_posterior=True)
    assert_trace(out, oracle_trace(C1, alg, prim, sec, llr, synd), "two shards")
    g.close()
