"""GPU parity of the frame-per-lane layout (Graph(H, layout="frame_per_lane"),
decoder_fpl.hip) against the CPU oracle — never against another plan.  The bar
is tests/test_gpu_parity.py's: hard bits, iteration counts, syndromes_match
and posterior LLRs bitwise.

A tile is 64 frames, one per lane; a frame that has exited is masked in every
kernel that writes its outputs, so the tests mix early and capped frames
inside each tile, cut batches into several chunks of tiles, and walk the exit
edges, the special LLR values and the row structures of tests/shape_codes.py.
"""
import gzip
import sys
import time

import numpy as np
import pytest

import qkd_ldpc_v_amd as Q
import shape_codes as S
from conftest import bits_equal_nan, diag_env, kat, load_fixture, matrix_path
from oracle import pyoracle as P
from oracle.pyoracle import Oracle
from test_dropin import oracle_trials
from test_gpu_parity import ALGS, frames
from test_gpu_shapes import QBER as SHAPE_QBER

pytestmark = pytest.mark.gpu

DBL_MAX = sys.float_info.max
C1, C4, C5 = "c1_n1024_m220.alist", "c4s_n102400_m32001.alist", "c5_n10240_m2048.sp2"
SPA, OMSA, AOMSA = ALGS[0], ALGS[3], ALGS[5]
_graphs, _oracles, _refs = {}, {}, {}


def matrix(name):
    return S.CODES[name]() if name in S.CODES else load_fixture(name)


def graph(name):
    if name not in _graphs:
        _graphs[name] = Q.Graph(matrix(name), layout="frame_per_lane")
        assert _graphs[name].plan(0, Q.SPA)["variant"] == "fpl"
    return _graphs[name]


def oracle(name):
    if name not in _oracles:
        _oracles[name] = Oracle(matrix(name))
    return _oracles[name]


def oracle_decode(name, alg, prim, sec, llr, synd, max_it=50, thr_on=True, key=None):
    """The oracle's (bits, iterations, ok, posterior); computed once per `key`
    and shared (read-only) by the tests that decode the same input."""
    if key is not None and key in _refs:
        return _refs[key]
    O = oracle(name)
    ref = O.decode_batch(O.params(alg, max_it, thr_on, 100.0, prim, sec), llr, synd, threads=16, posterior=True)
    for r in ref:
        r.setflags(write=False)
    if key is not None:
        _refs[key] = ref
    return ref


def assert_equal(out, ref, what):
    ob, oi, ok, op = ref
    bad = [f for f in range(ob.shape[0])
           if not (np.array_equal(out.bits[f], ob[f]) and out.iterations[f] == oi[f] and out.synd_ok[f] == ok[f]
                   and bits_equal_nan(out.posterior[f], op[f]))]
    assert not bad, (f"{what}: {len(bad)}/{ob.shape[0]} frames differ; first {bad[0]}: gpu it="
                     f"{out.iterations[bad[0]]} ok={out.synd_ok[bad[0]]} / oracle it={oi[bad[0]]} ok={ok[bad[0]]}; "
                     f"bit diffs={int((out.bits[bad[0]] != ob[bad[0]]).sum())}")


def assert_parity(name, alg, prim, sec, llr, synd, max_it=50, thr_on=True, key=None):
    out = graph(name).decode(Q.Params(alg, max_it, thr_on, 100.0, prim, sec), llr, synd, posterior=True)
    ref = oracle_decode(name, alg, prim, sec, llr, synd, max_it, thr_on, key)
    assert_equal(out, ref, f"{name} alg={alg} cap={max_it} thr={thr_on}")
    return out, ref


# ---- 1. KAT: one lane of one tile -------------------------------------------------------------------
def test_kat_johnson(gpu_available):
    K = kat()
    H = load_fixture("kat_n6_m4.dense")
    lp = Q.log_p(K["qber"])
    llr = np.where(np.array(K["bob"]) != 0, -lp, lp)
    s = H.syndrome(np.array(K["alice"], np.uint8))
    out = graph("kat_n6_m4.dense").decode(Q.Params(K["algorithm"], K["max_iterations"], K["thr_enabled"], K["thr"]),
                                          llr, s, posterior=True)
    E = K["expected"]
    assert int(out.iterations[0]) == E["iterations"] and bool(out.synd_ok[0]) == E["syndromes_match"]
    assert out.bits[0].tolist() == E["bob_solution"]
    assert bits_equal_nan(out.posterior[0], np.array(E["posterior_iteration_1"]))


# ---- 2. two full tiles and a two-lane tail, early and capped frames in every tile ---------------------
@pytest.mark.parametrize("alg,prim,sec", ALGS)
def test_tiles_and_tail(gpu_available, alg, prim, sec):
    """130 frames: every full tile (in index order, frames 0-63 and 64-127)
    holds at least 8 frames that stop before the cap and 8 that reach it, so
    settled lanes sit beside running ones through most of the decode.  Decoded
    as dealt (claim order), in index order, and as three chunks of one tile."""
    _, _, llr, synd = frames(load_fixture(C1), 0.02, 130, seed=1)
    key = ("tiles", alg)
    _, (ob, oi, ok, op) = assert_parity(C1, alg, prim, sec, llr, synd, key=key)
    for t in (0, 1):
        tile = oi[64 * t:64 * t + 64]
        early, capped = int((tile < 50).sum()), int((tile == 50).sum())
        assert early >= 8 and capped >= 8, f"alg={alg} tile {t}: {early} early, {capped} at the cap"
    with diag_env(QLDPC_ORDER="0"):
        assert_parity(C1, alg, prim, sec, llr, synd, key=key)
    with diag_env(QLDPC_FPL_TILES="1"):
        assert_parity(C1, alg, prim, sec, llr, synd, key=key)


# ---- 3. exit edges ----------------------------------------------------------------------------------
@pytest.mark.parametrize("alg,prim,sec", [SPA, OMSA, AOMSA])
def test_exit_edges(gpu_available, alg, prim, sec):
    """Iteration caps 1-3 (the closing parity follows the only bit pass),
    error-free frames with +-inf LLRs (AOMSA leaves in iteration 0 with the
    channel decision and an all-zero posterior, SPA / OMSA in iteration 1) and
    frames that converge in a few iterations."""
    H = load_fixture(C1)
    for max_it in (1, 2, 3):
        _, _, llr, synd = frames(H, 0.02, 5, seed=700 + max_it)
        for thr_on in (True, False):
            assert_parity(C1, alg, prim, sec, llr, synd, max_it=max_it, thr_on=thr_on)
    _, _, llr, synd = frames(H, 1e-6, 5, seed=750)
    assert np.isinf(llr).all()
    out, (ob, oi, ok, op) = assert_parity(C1, alg, prim, sec, llr, synd)
    assert out.synd_ok.all()
    assert (oi == 1).all()  # (left in the first iteration: AOMSA before its bit pass, SPA / OMSA after it)
    if alg == Q.AOMSA:
        assert not op.any() and not out.posterior.any()
    _, _, llr, synd = frames(H, 0.003, 5, seed=751)
    assert_parity(C1, alg, prim, sec, llr, synd)


# ---- 4. special LLR values --------------------------------------------------------------------------
@pytest.mark.parametrize("thr_on", [True, False])
@pytest.mark.parametrize("alg,prim,sec", ALGS)
def test_special_llrs(gpu_available, alg, prim, sec, thr_on):
    H = load_fixture(C1)
    _, _, llr, synd = frames(H, 0.02, 16, seed=60 + alg)
    llr = llr * np.random.default_rng(61 + alg).uniform(0.6, 1.4, llr.shape)
    llr[::2, :8] = [1e-4, -1e-4, 0.0, -0.0, DBL_MAX, np.inf, -np.inf, np.nan]
    assert_parity(C1, alg, prim, sec, llr, synd, thr_on=thr_on)


# ---- 5. row structures ------------------------------------------------------------------------------
ROW_CASES = ["degree1_rows", "empty_row_first", "empty_row_last", "long_row33", "long_row41", "degree510_bit",
             "short_rows", "split_k4_isolated"]


@pytest.mark.parametrize("alg,prim,sec", [SPA, OMSA, AOMSA])
@pytest.mark.parametrize("case", ROW_CASES)
def test_row_structures(gpu_available, case, alg, prim, sec):
    """One-edge rows, an empty first / last row, rows past the register cap of
    the check-node pass (33 and 41 edges), a bit of degree 510, many short rows,
    isolated bits: the QBERs (and so the spreads) recorded in tests/test_gpu_shapes.py."""
    q, own = SHAPE_QBER[case]
    _, _, llr, synd = frames(matrix(case), own.get(alg, q), 9 if case == "split_k4_isolated" else 12, seed=1)
    assert_parity(case, alg, prim, sec, llr, synd)


def test_empty_row_between_two_others(gpu_available):
    """An empty check in the middle (the register layouts refuse it): parity 0,
    so a frame whose syndrome bit there is 1 can never match."""
    H = S.empty_row(200)
    name = "empty_row_mid"
    _graphs[name] = Q.Graph(H, layout="frame_per_lane")
    _oracles[name] = Oracle(H)
    _, _, llr, synd = frames(H, 0.010, 8, seed=1)
    synd = synd.copy()
    synd[::2, 200] = 1
    for alg, prim, sec in (SPA, OMSA, AOMSA):
        out, _ = assert_parity(name, alg, prim, sec, llr, synd, max_it=12)
        assert not out.synd_ok[::2].any()


# ---- 6. n = 102,400 ---------------------------------------------------------------------------------
@pytest.mark.parametrize("alg,prim,sec", [SPA, AOMSA])
def test_c4_100k(gpu_available, alg, prim, sec):
    _, _, llr, synd = frames(load_fixture(C4), 0.038, 6, seed=9)
    _, (ob, oi, ok, op) = assert_parity(C4, alg, prim, sec, llr, synd)
    assert oi.min() < 50


# ---- 7. entries -------------------------------------------------------------------------------------
def test_device_entry_on_a_side_stream(gpu_available):
    """qldpc_decode_batch_device on a non-default stream, no posterior; 70
    frames are dealt to two tiles in the claim order, which the graph reports."""
    import torch

    H = load_fixture(C1)
    g = graph(C1)
    alg, prim, sec = OMSA
    _, _, llr, synd = frames(H, 0.02, 70, seed=31)
    dev = torch.device("cuda:0")
    st = torch.cuda.Stream(device=dev)
    tl, ts = torch.from_numpy(llr).to(dev), torch.from_numpy(synd).to(dev)
    bits = torch.empty((70, H.n), dtype=torch.uint8, device=dev)
    it = torch.empty(70, dtype=torch.int32, device=dev)
    ok = torch.empty(70, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    g.decode_device(Q.Params(alg, 50, True, 100.0, prim, sec), tl, ts, bits, it, ok, None, stream=st)
    st.synchronize()
    ob, oi, ook, _ = oracle_decode(C1, alg, prim, sec, llr, synd)
    assert np.array_equal(bits.cpu().numpy(), ob)
    assert np.array_equal(it.cpu().numpy().astype(np.uint32), oi) and np.array_equal(ok.cpu().numpy(), ook)
    order, weight = g.last_claim_order(stream=st)
    assert sorted(order.tolist()) == list(range(70)) and np.all(np.diff(weight[order]) >= 0)
    # one tile: dealt in index order, reported as count 0
    g.decode_device(Q.Params(alg, 50, True, 100.0, prim, sec), tl[:5], ts[:5], bits[:5], it[:5], ok[:5], None,
                    stream=st)
    st.synchronize()
    assert g.last_claim_order(stream=st) == (None, None)
    assert np.array_equal(bits[:5].cpu().numpy(), ob[:5])


def test_fused_entry_without_llr_workspace(gpu_available):
    """qldpc_qkd_ldpc_batch_device with d_llr_ws == NULL: the frames' LLRs go
    through the internal workspace (the palette codes are the register kernels')."""
    import torch

    H = load_fixture(C5)
    g = graph(C5)
    batch = 20
    a, b, llr, s = frames(H, 0.0156, batch, 5)
    q = int(H.n * 0.0156) / H.n
    dev = torch.device("cuda:0")
    ta, tb = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    lp = torch.full((batch,), Q.log_p(q), dtype=torch.float64, device=dev)
    syn_ws = torch.empty((batch, H.m), dtype=torch.uint8, device=dev)
    bits = torch.empty((batch, H.n), dtype=torch.uint8, device=dev)
    it = torch.empty(batch, dtype=torch.int32, device=dev)
    ok = torch.empty(batch, dtype=torch.uint8, device=dev)
    km = torch.empty(batch, dtype=torch.uint8, device=dev)
    alg, prim, sec = Q.AOMSA, 0.7, 0.99
    g.qkd_ldpc_device(Q.Params(alg, 50, True, 100.0, prim, sec), ta, tb, lp, None, syn_ws, bits, it, ok, km)
    torch.cuda.synchronize()
    assert np.array_equal(syn_ws.cpu().numpy(), s)
    ob, oi, ook, _ = oracle_decode(C5, alg, prim, sec, llr, s)
    assert np.array_equal(bits.cpu().numpy(), ob)
    assert np.array_equal(it.cpu().numpy().astype(np.uint32), oi) and np.array_equal(ok.cpu().numpy(), ook)
    assert np.array_equal(km.cpu().numpy(), (ob == a).all(axis=1).astype(np.uint8))


def test_rate_adapted_trials_blocking_and_submitted(gpu_available):
    """qldpc_run_trials with a rate plan, and the same trials through
    submit / wait, chunks of 5 over both pipeline slots: every trial equals
    the oracle's run_trial.  runtime_us is each trial's share of its chunk's
    window in proportion to its decode span (frame_clk: the first check-node
    pass to the settle step that ends the frame): finite and positive, and the
    windows of one device do not overlap and lie inside the call, so their
    sum — the sum of the shares — is at most the call's wall time."""
    H = load_fixture(C5)
    u = np.array(gzip.open(matrix_path("c5_n10240_m2048.untp")).read().split(), np.int32)
    punct, short, _ = Q.adapt_code_rate(H.n, H.m, 0.0156, 0.06, 1.39, u, Q.xoshiro_state(5555))
    g = graph(C5)
    plan = g.rate_plan(punct, short)
    alg, prim, sec, qber, seed_add = Q.AOMSA, 0.7, 0.99, 0.0156, 2
    seeds = P.trial_seeds(5555, 11)
    p = Q.Params(alg, 50, True, 100.0, prim, sec)
    want = oracle_trials(H, alg, prim, sec, qber, 50, [(int(s) + seed_add) & 0xFFFFFFFFFFFFFFFF for s in seeds],
                         punct, short)
    with diag_env(QLDPC_TRIAL_CHUNK="5"):
        g.run_trials(p, qber, seeds[:2], seed_add=seed_add, plan=plan)  # warm: workspaces, generator tables
        t0 = time.perf_counter()
        blocking = g.run_trials(p, qber, seeds, seed_add=seed_add, plan=plan)
        wall_us = (time.perf_counter() - t0) * 1e6
        submitted = g.submit_trials(p, qber, seeds, seed_add=seed_add, plan=plan).wait()
    for out in (blocking, submitted):
        assert [(int(a), int(b), int(c)) for a, b, c in zip(out.iterations, out.synd_ok, out.keys_match)] == want
        assert out.accurate_qber == int(H.n * qber) / H.n
        assert np.all(np.isfinite(out.runtime_us)) and np.all(out.runtime_us > 0)
    assert blocking.runtime_us.sum() <= wall_us


def test_kernel_timing_brackets_the_launch_sequence(gpu_available):
    import torch

    H = load_fixture(C1)
    g = Q.Graph(H, layout="frame_per_lane")
    g.set_kernel_timing(True)
    _, _, llr, synd = frames(H, 0.02, 70, seed=32)
    dev = torch.device("cuda:0")
    tl, ts = torch.from_numpy(llr).to(dev), torch.from_numpy(synd).to(dev)
    bits = torch.empty((70, H.n), dtype=torch.uint8, device=dev)
    it = torch.empty(70, dtype=torch.int32, device=dev)
    ok = torch.empty(70, dtype=torch.uint8, device=dev)
    g.decode_device(Q.Params(Q.SPA, 50, True, 100.0), tl, ts, bits, it, ok)
    ms = g.last_decode_kernel_ms()
    assert np.isfinite(ms) and ms > 0
    ob, oi, ook, _ = oracle_decode(C1, Q.SPA, 0.0, 0.0, llr, synd)
    assert np.array_equal(bits.cpu().numpy(), ob) and np.array_equal(it.cpu().numpy().astype(np.uint32), oi)
    g.close()


def test_two_shards_on_one_device(gpu_available):
    """devices=[0, 0]: a 70-frame batch as two slices of 35, one host thread,
    stream and workspace each."""
    H = load_fixture(C1)
    g = Q.Graph(H, devices=[0, 0], layout="frame_per_lane")
    assert g.info()["devices"] == 2 and g.plan(0, Q.SPA)["variant"] == "fpl"
    # the check-node pass's grid for one tile: four rows per workgroup, per class of row lengths
    assert (H.m + 3) // 4 <= g.plan(0, Q.SPA)["workgroups"] <= (H.m + 3) // 4 + 8
    alg, prim, sec = AOMSA
    _, _, llr, synd = frames(H, 0.02, 70, seed=33)
    out = g.decode(Q.Params(alg, 50, True, 100.0, prim, sec), llr, synd, posterior=True)
    assert_equal(out, oracle_decode(C1, alg, prim, sec, llr, synd), "two shards")
    g.close()
