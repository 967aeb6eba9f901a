"""Symmetric blind reconciliation on the GPU: Bob's selection of each failed
frame's least reliable positions (qldpc_select_positions*), Alice's answer
(qldpc_disclose_positions*), Bob's positions round
(qldpc_reconcile_positions_round*) and blind.symmetric_reconcile.

The selection is checked bit for bit against numpy (symmetric_ref.np_select:
a lexsort on the posterior's 63 magnitude bits and the index), on synthetic
posteriors built for the ways a radix select can go wrong.  The rounds are
checked against the CPU oracle on numpy's pinned LLRs, on test_gpu_blind's
fixture (C1, 60 punctured, 4 shortened, 70 frames at QBER 0.016, 20 iterations,
20 positions per round) and, without a plan, on test_gpu_parties' C1 frames at
QBER 0.02."""
import functools
import sys

import numpy as np
import pytest

import qkd_ldpc_v_amd as Q
from conftest import diag_env, load_fixture
from oracle.pyoracle import Oracle
from qkd_ldpc_v_amd import privacy
from symmetric_ref import excluded, np_select, np_symmetric
from test_gpu_blind import BATCH, CAP, PUNCT, QBER, ROUND_ALGS, SHORT, STEP, c1_oracle, fixture, oracle_params
from test_gpu_parties import assert_same, c1_frames, c1_graphs, cuda

pytestmark = pytest.mark.gpu

C1 = "c1_n1024_m220.alist"
N = 1024
DBL_MAX = sys.float_info.max
FILL = -7  # the sentinel of position buffers
LISTED = np.array([6, 0, 8, 3, 1, 5, 2], np.int32)  # 7 of 9 frames, scrambled; 4 and 7 are not listed


# ---- 1. the selection -----------------------------------------------------------------
def bits_to_f64(u):
    return np.ascontiguousarray(u, np.uint64).view(np.float64)


@functools.lru_cache(maxsize=None)
def synthetic_posteriors(n=N):
    """9 rows: 0: three magnitudes (massive ties, a threshold bucket far larger
    than any count); 1: keys that differ in the lowest byte only; 2: keys that
    differ in the top (exponent) byte only; 3: +-0, denormals, 1e-4, +-DBL_MAX,
    +-inf and NaNs mixed; 5: one value everywhere (pure index order); 6: few
    distinct values around ordinary ones; 4, 7, 8: continuous."""
    rng = np.random.Generator(np.random.PCG64(21))
    sign = lambda: rng.integers(0, 2, n).astype(np.uint64) << np.uint64(63)  # noqa: E731
    post = rng.normal(0.0, 10.0, (9, n))
    post[0] = rng.choice([0.37, 2.5, 41.0], n) * rng.choice([-1.0, 1.0], n)
    post[1] = bits_to_f64(np.uint64(0x4005BF0A8B145700) | rng.integers(0, 256, n).astype(np.uint64) | sign())
    post[2] = bits_to_f64((rng.integers(0, 128, n).astype(np.uint64) << np.uint64(56)) | np.uint64(0x000FEDCBA9876543)
                          | sign())
    specials = np.array([0.0, -0.0, 5e-324, -5e-324, 2.2e-308 / 3, 1e-4, -1e-4, DBL_MAX, -DBL_MAX, np.inf, -np.inf,
                         np.nan, 1.5, -1.5])
    post[3] = rng.choice(specials, n)
    payload = rng.integers(1, 1 << 20, post[3, ::97].size).astype(np.uint64)
    post[3, ::97] = bits_to_f64(np.uint64(0xFFF8000000000000) | payload)  # negative NaNs with payloads
    post[5] = 1e-4
    post[6] = np.round(post[6])  # about 60 distinct magnitudes
    post.setflags(write=False)
    return post


def np_positions(post, frames, first, count, short, history):
    """Expected pos after a select over `frames`: FILL, the histories, the selections."""
    pos = np.full(history.shape, FILL, np.int32)
    for f in frames:
        pos[f, :first] = history[f, :first]
        pos[f, first:first + count] = np_select(post[f], excluded(post.shape[1], short, history[f, :first]), count)
    return pos


def histories(batch, n, cap, short, seed=4):
    """Per frame a random order of the positions that are not shortened: a history of any length up to cap."""
    rng = np.random.Generator(np.random.PCG64(seed))
    free = np.setdiff1d(np.arange(n), [] if short is None else short)
    return np.stack([rng.permutation(free)[:cap] for _ in range(batch)]).astype(np.int32)


def device_select(g, plan, post, frames, first, count, history):
    import torch

    pos = np.full(history.shape, FILL, np.int32)
    pos[frames, :first] = history[frames, :first]
    d_pos, d_post = cuda(pos), cuda(np.array(post))  # (a writable copy: the shared rows are read-only)
    g.select_positions_device(d_post, cuda(np.asarray(frames, np.int32)), first, count, d_pos, plan=plan)
    torch.cuda.synchronize()
    assert np.array_equal(d_post.cpu().numpy().view(np.uint64), post.view(np.uint64)), "the posteriors were written to"
    return d_pos.cpu().numpy()


@pytest.mark.parametrize("with_plan", [True, False], ids=["plan", "no plan"])
@pytest.mark.parametrize("first", [0, 20])
def test_select_against_numpy(gpu_available, with_plan, first):
    _, g = c1_graphs()
    plan, short = (g.rate_plan(PUNCT, SHORT), SHORT) if with_plan else (None, None)
    post = synthetic_posteriors()
    hist = histories(9, N, N, short)
    every = N - (SHORT.size if with_plan else 0) - first
    got = {}
    for count in (1, 20, 63, 64, 65, every):
        got[count] = device_select(g, plan, post, LISTED, first, count, hist)
        want = np_positions(post, LISTED, first, count, short, hist)
        bad = np.flatnonzero((got[count] != want).any(axis=1))
        # (the whole array: unlisted rows and the columns outside [first, first + count) keep FILL)
        assert bad.size == 0, f"count {count}, first {first}: rows {bad.tolist()} differ"
    assert np.array_equal(got[20][:, :first + 20], got[64][:, :first + 20]), "a shorter selection is a prefix"
    chosen = got[every][LISTED, first:first + every]
    assert (np.sort(chosen, axis=1) == np.sort(np.stack([np.setdiff1d(np.arange(N), np.concatenate(
        [hist[f, :first], SHORT if with_plan else []])) for f in LISTED]), axis=1)).all(), "every candidate, once"
    if with_plan:
        assert not np.isin(got[65][LISTED, first:first + 65], SHORT).any(), "a shortened position was chosen"
        assert np.isin(PUNCT, chosen[0]).sum() >= PUNCT.size - first, "punctured positions are candidates"
        # row 5 is one value everywhere: index order, so the punctured position 0 comes first unless it is history
        f5 = got[20][5, first:first + 20]
        assert f5[0] == min(set(range(N)) - set(SHORT.tolist()) - set(hist[5, :first].tolist()))


def test_select_beyond_the_limit(gpu_available):
    """count = QLDPC_SELECT_MAX + 1: QLDPC_EUNSUP, and nothing is launched."""
    import torch

    _, g = c1_graphs()
    d_pos = torch.full((9, Q.SELECT_MAX + 8), FILL, dtype=torch.int32, device="cuda")
    with pytest.raises(Q.QLDPCError, match="EUNSUP.*QLDPC_SELECT_MAX") as e:
        g.select_positions_device(cuda(np.array(synthetic_posteriors())), cuda(LISTED), 0, Q.SELECT_MAX + 1, d_pos)
    assert e.value.code == -5
    torch.cuda.synchronize()
    assert (d_pos.cpu().numpy() == FILL).all()


@pytest.mark.parametrize("with_plan", [True, False], ids=["plan", "no plan"])
def test_select_smaller_than_a_wave(gpu_available, with_plan):
    """n = 10: every count, with ties, on every frame."""
    H = load_fixture("u_n10_m5.dense")
    g = Q.Graph(H)
    punct, short = np.array([0, 9], np.int32), np.array([4], np.int32)
    plan = g.rate_plan(punct, short) if with_plan else None
    short = short if with_plan else None
    rng = np.random.Generator(np.random.PCG64(8))
    post = np.round(rng.normal(0.0, 2.0, (5, 10)))
    post[3] = [np.nan, -0.0, 0.0, np.inf, 5e-324, -np.inf, 1e-4, -1e-4, DBL_MAX, -3.0]
    hist = histories(5, 10, 10, short)
    frames = np.array([4, 0, 3, 1, 2], np.int32)
    for first in (0, 3):
        for count in range(1, 10 - (1 if with_plan else 0) - first + 1):
            got = device_select(g, plan, post, frames, first, count, hist)
            assert np.array_equal(got, np_positions(post, frames, first, count, short, hist)), (first, count)


# ---- 2. Alice's answer ------------------------------------------------------------------
def test_disclose_positions(gpu_available):
    import torch

    ga, _ = c1_graphs()
    plan = ga.rate_plan(PUNCT, SHORT)
    rng = np.random.Generator(np.random.PCG64(12))
    stride = N + 24
    ext = rng.integers(0, 4, (9, stride)).astype(np.uint8)  # (bit 0 of the byte counts; the bytes past n are never read)
    pos = histories(9, N, 100, None, seed=6)
    d_ext, d_pos = cuda(ext), cuda(pos)
    for frames, first, count, pl in ((LISTED, 0, 20, plan), (LISTED, 20, 65, None), (np.arange(9), 0, 100, plan),
                                     (np.array([8]), 99, 1, None), (np.array([3, 0]), 37, 63, plan)):
        out = torch.full((len(frames), count), 7, dtype=torch.uint8, device="cuda")
        ga.disclose_positions_device(d_ext, cuda(frames.astype(np.int32)), d_pos, first, count, out, plan=pl)
        torch.cuda.synchronize()
        want = np.stack([ext[f, pos[f, first:first + count]] & 1 for f in frames])
        assert np.array_equal(out.cpu().numpy(), want), (frames, first, count)
    out = torch.full((5, 20), 7, dtype=torch.uint8, device="cuda")  # n_list below the list's capacity
    ga.disclose_positions_device(d_ext, cuda(LISTED[:5]), d_pos, 0, 20, out, n_list=3)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(got[:3], np.stack([ext[f, pos[f, :20]] & 1 for f in LISTED[:3]])) and (got[3:] == 7).all()


# ---- 3. the positions round against the oracle ---------------------------------------------
@functools.lru_cache(maxsize=None)
def sym_rounds(alg, prim, sec, max_rounds=None):
    """np_symmetric on the blind fixture (at most 100 positions per frame), with
    its non-degeneracy asserted: at least 2 frames still fail after round 0, at
    least 2 newly decode in round 1 and at least 2 go on to round 2."""
    _, _, _, _, ext, syn, llr0 = fixture()
    res = np_symmetric(c1_oracle(), oracle_params(alg, prim, sec), llr0, syn, ext, SHORT, STEP, max_rounds, 100)
    states = res[0]
    ok0, ok1 = states[0][2], states[1][2]
    assert int((ok0 == 0).sum()) >= 2 and int(((ok0 == 0) & (ok1 == 1)).sum()) >= 2, (alg, ok0.sum(), ok1.sum())
    assert max_rounds == 1 or (len(states) >= 3 and int((ok1 == 0).sum()) >= 2)
    return res


def device_positions_round(g, par, plan, frames, n_disc, positions, ext, prev, bob, lp, syn, posterior=True):
    """One qldpc_reconcile_positions_round_device call on outputs pre-filled with prev -> the whole arrays."""
    import torch

    batch = bob.shape[0]
    lp = np.array(np.broadcast_to(np.asarray(lp, np.float64), (batch,)))
    frames = np.asarray(frames, np.int32)
    vals = np.stack([ext[f, positions[f, :n_disc]] & 1 for f in frames]) if frames.size else np.empty((0, n_disc), np.uint8)
    d_syn = cuda(syn)
    bits, ok, it = cuda(prev[0]), cuda(prev[2]), cuda(prev[1].astype(np.int32))
    post = cuda(prev[3]) if posterior else None
    g.reconcile_positions_round_device(par, cuda(bob), cuda(lp), d_syn, cuda(frames), n_disc, cuda(positions),
                                       cuda(vals), bits, it, ok, plan=plan, posterior=post)
    torch.cuda.synchronize()
    assert np.array_equal(d_syn.cpu().numpy(), syn), "the received syndrome was written to"
    return Q.DecodeOutput(bits.cpu().numpy(), it.cpu().numpy().astype(np.uint32), ok.cpu().numpy(),
                          post.cpu().numpy() if posterior else None)


def check_sym_rounds(g, alg, prim, sec, which):
    _, bob, _, lp, ext, syn, _ = fixture()
    states, lists, _, _, _, positions = sym_rounds(alg, prim, sec)
    plan = g.rate_plan(PUNCT, SHORT)
    par = Q.Params(alg, CAP, True, 100.0, prim, sec)
    for r in which:
        out = device_positions_round(g, par, plan, lists[r - 1], STEP * r, positions, ext, states[r - 1], bob, lp, syn)
        assert_same(out, states[r], f"round {r} ({lists[r - 1].size} frames)")  # listed and unlisted rows alike


def test_fixture_pins_a_key_bit_bob_has_wrong(gpu_available):
    """Among round 1's pins there are key positions (class 0) where Alice's bit
    differs from Bob's, and punctured ones: the pins are of any class."""
    _, _, _, _, ext, _, llr0 = fixture()
    _, lists, _, _, _, positions = sym_rounds(*ROUND_ALGS[0])
    f = lists[0]
    p = positions[f, :STEP].astype(np.int64)
    is_key = ~np.isin(p, np.concatenate([PUNCT, SHORT]))
    bob_bit = np.take_along_axis(llr0[f], p, axis=1) < 0
    alice_bit = np.take_along_axis(ext[f], p, axis=1) == 1
    assert int((is_key & (bob_bit != alice_bit)).sum()) >= 2 and int(np.isin(p, PUNCT).sum()) >= 2
    assert not np.isin(p, SHORT).any()


@pytest.mark.parametrize("alg,prim,sec", ROUND_ALGS)
def test_positions_rounds_against_the_oracle(gpu_available, alg, prim, sec):
    _, gb = c1_graphs()
    assert gb.plan(0, alg)["variant"] == "v2"
    check_sym_rounds(gb, alg, prim, sec, (1, 2))


@pytest.mark.parametrize("layout", ["frame_per_lane", "v1"])
def test_positions_round_other_layouts(gpu_available, layout):
    H = load_fixture(C1)
    alg, prim, sec = ROUND_ALGS[0]
    if layout == "v1":
        with diag_env(QLDPC_VARIANT="v1"):  # (read at graph creation)
            g = Q.Graph(H)
        assert g.plan(0, alg)["variant"] == "reg_lds"
    else:
        g = Q.Graph(H, layout=layout)
        assert g.plan(0, alg)["variant"] == "fpl"
    check_sym_rounds(g, alg, prim, sec, (1,))


def test_no_positions_is_a_fixed_order_round_without_disclosure(gpu_available):
    """n_disc == 0 over a list: qldpc_reconcile_round_device with n_disc == 0, byte for byte."""
    import torch

    _, gb = c1_graphs()
    _, bob, _, lp, ext, syn, _ = fixture()
    plan = gb.rate_plan(PUNCT, SHORT)
    alg, prim, sec = ROUND_ALGS[0]
    par = Q.Params(alg, CAP, True, 100.0, prim, sec)
    frames = np.array([5, 69, 0, 33], np.int32)
    junk = (np.full((BATCH, N), 7, np.uint8), np.full(BATCH, 77, np.uint32), np.full(BATCH, 7, np.uint8),
            np.full((BATCH, N), -7.0))
    bits, ok, it, post = cuda(junk[0]), cuda(junk[2]), cuda(junk[1].astype(np.int32)), cuda(junk[3])
    gb.reconcile_round_device(par, cuda(bob), cuda(np.full(BATCH, lp)), cuda(syn), plan, cuda(frames), None, None, bits,
                              it, ok, posterior=post)
    torch.cuda.synchronize()
    want = (bits.cpu().numpy(), it.cpu().numpy().astype(np.uint32), ok.cpu().numpy(), post.cpu().numpy())
    positions = np.full((BATCH, 8), -1, np.int32)
    out = device_positions_round(gb, par, plan, frames, 0, positions, ext, junk, bob, lp, syn)
    assert_same(out, want, "a positions round without positions")
    assert (out.bits[1] == 7).all() and out.iterations[1] == 77 and (out.posterior[1] == -7.0).all()
    assert_same(Q.DecodeOutput(*(x[frames] for x in want)), tuple(x[frames] for x in sym_rounds(alg, prim, sec)[0][0]),
                "round 0 again")


# ---- 4. without a plan: C1 unadapted at QBER 0.02 ------------------------------------------
@functools.lru_cache(maxsize=None)
def noplan_rounds(max_rounds=None):
    alice, _, _, llr, syn = c1_frames()
    O = Oracle(load_fixture(C1))
    res = np_symmetric(O, O.params(Q.SPA, CAP, True, 100.0, 0.0, 0.0), llr, syn, alice, None, STEP, max_rounds, 100)
    ok0, ok1 = res[0][0][2], res[0][1][2]
    assert int((ok0 == 0).sum()) >= 2 and int(((ok0 == 0) & (ok1 == 1)).sum()) >= 2, (ok0.sum(), ok1.sum())
    return res


def test_positions_round_without_a_plan(gpu_available):
    _, gb = c1_graphs()
    alice, bob, lp, _, syn = c1_frames()
    states, lists, _, _, _, positions = noplan_rounds()
    par = Q.Params(Q.SPA, CAP, True, 100.0)
    for r in (1, 2)[:len(lists)]:
        out = device_positions_round(gb, par, None, lists[r - 1], STEP * r, positions, alice, states[r - 1], bob, lp, syn)
        assert_same(out, states[r], f"no plan, round {r} ({lists[r - 1].size} frames)")
    out = device_positions_round(gb, par, None, lists[0][:3], STEP, positions, alice, states[0], bob, lp, syn,
                                 posterior=False)
    f = lists[0][:3]
    assert np.array_equal(out.bits[f], states[1][0][f]) and np.array_equal(out.synd_ok[f], states[1][2][f])


# ---- 5. host entries: two shards on one GPU --------------------------------------------------
def test_host_entries_equal_device_entries(gpu_available):
    H = load_fixture(C1)
    g2 = Q.Graph(H, devices=[0, 0])
    _, gb = c1_graphs()
    alg, prim, sec = ROUND_ALGS[0]
    par = Q.Params(alg, CAP, True, 100.0, prim, sec)
    plan2, planb = g2.rate_plan(PUNCT, SHORT), gb.rate_plan(PUNCT, SHORT)
    _, bob, _, lp, ext, syn, _ = fixture()
    states, lists, _, _, _, positions = sym_rounds(alg, prim, sec)
    # the selection, on the synthetic rows: uneven shards (7 frames over 2), one frame, none
    post = synthetic_posteriors()
    for pl2, plb, short in ((plan2, planb, SHORT), (None, None, None)):
        hist = histories(9, N, 90, short)
        for frames, first, count in ((LISTED, 20, 65), (LISTED[:1], 0, 20), (LISTED[:0], 0, 20)):
            pos = np.full(hist.shape, FILL, np.int32)
            pos[frames, :first] = hist[frames, :first]
            assert g2.select_positions(post, frames, first, count, pos, plan=pl2) is pos
            assert np.array_equal(pos, np_positions(post, frames, first, count, short, hist)), (frames, first, count)
            if frames.size:
                assert np.array_equal(pos, device_select(gb, plb, post, frames, first, count, hist))
    # Alice's answer and Bob's round, on the fixture's round 1
    for size in (5, 1, 0):
        frames = lists[0][-size:] if size else lists[0][:0]
        wide = np.concatenate([ext, np.full((BATCH, 8), 1, np.uint8)], axis=1)  # rows of n + 8 bytes
        vals = g2.disclose_positions(wide, frames, positions, 0, STEP, plan=plan2)
        want_vals = np.stack([ext[f, positions[f, :STEP]] for f in frames]) if size else np.empty((0, STEP), np.uint8)
        assert vals.shape == (size, STEP) and np.array_equal(vals, want_vals)
        prev = Q.DecodeOutput(*(x.copy() for x in states[0]))
        out = g2.reconcile_positions_round(par, bob, lp, syn, frames, STEP, positions, vals, plan=plan2, out=prev)
        want = tuple(x.copy() for x in states[0])
        for w, s in zip(want, states[1]):
            w[frames] = s[frames]
        assert out is prev
        assert_same(out, want, f"host round, {size} frames")
        assert_same(device_positions_round(gb, par, planb, frames, STEP, positions, ext, states[0], bob, lp, syn), want,
                    f"device round, {size} frames")
    with pytest.raises(Q.QLDPCError, match="EINVAL.*twice"):
        g2.select_positions(post, [3, 3], 0, 5, np.full((9, 8), -1, np.int32), plan=plan2)
    with pytest.raises(Q.QLDPCError, match="EINVAL.*candidates"):
        g2.select_positions(post, [3], 0, N - 3, np.full((9, N), -1, np.int32), plan=plan2)


# ---- 6. the whole exchange ---------------------------------------------------------------
def assert_exchange(res, ref, ext):
    states, lists, rounds, disclosed, iters, positions = ref
    assert np.array_equal(res.rounds, rounds) and np.array_equal(res.disclosed, disclosed)
    assert np.array_equal(res.synd_ok, states[-1][2]) and np.array_equal(res.bits, states[-1][0])
    assert np.array_equal(res.iterations, iters)
    assert res.positions.dtype == np.int32 and np.array_equal(res.positions, positions)
    for f in range(res.positions.shape[0]):  # -1 past disclosed[f]
        assert (res.positions[f, disclosed[f]:] == -1).all() and (res.positions[f, :disclosed[f]] >= 0).all()
    done = res.synd_ok == 1
    assert np.array_equal(res.bits[done], ext[done])


@pytest.mark.parametrize("max_rounds", [None, 1])
def test_symmetric_reconcile(gpu_available, max_rounds):
    ga, gb = c1_graphs()
    alg, prim, sec = ROUND_ALGS[0]
    alice, bob, fill, lp, ext, _, _ = fixture()
    ref = sym_rounds(alg, prim, sec, max_rounds)
    res = Q.symmetric_reconcile(ga, ga.rate_plan(PUNCT, SHORT), gb, gb.rate_plan(PUNCT, SHORT),
                                Q.Params(alg, CAP, True, 100.0, prim, sec), alice, bob, lp, fill, STEP,
                                max_rounds=max_rounds, max_disclosed=100, q=QBER)
    assert_exchange(res, ref, ext)
    assert np.array_equal(res.efficiency.view(np.uint64),
                          Q.blind_efficiency(N, 220, 60, 4, ref[3], QBER).view(np.uint64))
    assert res.rounds.max() == (1 if max_rounds else len(ref[1])) and len(ref[1]) >= (1 if max_rounds else 2)


@pytest.mark.parametrize("max_rounds", [None, 1])
def test_symmetric_reconcile_without_a_plan(gpu_available, max_rounds):
    ga, gb = c1_graphs()
    alice, bob, lp, _, _ = c1_frames()
    ref = noplan_rounds(max_rounds)
    res = Q.symmetric_reconcile(ga, None, gb, None, Q.Params(Q.SPA, CAP, True, 100.0), alice, bob, lp, None, STEP,
                                max_rounds=max_rounds, max_disclosed=100)
    assert_exchange(res, ref, alice)
    assert np.isnan(res.efficiency).all()


# ---- 7. closing: verification and privacy amplification after a symmetric run ------------------
def test_amplify_after_a_symmetric_run(gpu_available):
    """Disclosed key positions stay in the key; secret_length removes them through
    leaked_bits.  Both sides amplify to the same bits wherever the tags agree."""
    import torch

    ga, gb = c1_graphs()
    alg, prim, sec = ROUND_ALGS[0]
    alice, bob, fill, lp, _, _, _ = fixture()
    plan_b = gb.rate_plan(PUNCT, SHORT)
    res = Q.symmetric_reconcile(ga, ga.rate_plan(PUNCT, SHORT), gb, plan_b, Q.Params(alg, CAP, True, 100.0, prim, sec),
                                alice, bob, lp, fill, STEP, max_rounds=1, q=QBER)
    n_key = plan_b.n_key
    d_key = torch.full((BATCH, n_key), 7, dtype=torch.uint8, device="cuda")
    gb.extract_key_device(plan_b, cuda(res.bits), d_key)
    torch.cuda.synchronize()
    key_b, key_a = d_key.cpu().numpy(), np.ascontiguousarray(alice[:, :n_key])
    equal = (key_a == key_b).all(axis=1)
    assert 2 <= int(equal.sum()) <= BATCH - 2, "one round leaves right and wrong keys"
    rng = np.random.Generator(np.random.PCG64(31))
    tag_seed = rng.integers(0, 2, n_key + 63).astype(np.uint8)
    ok = privacy.verified(privacy.tag(key_a, tag_seed), privacy.tag(key_b, tag_seed))
    assert np.array_equal(ok, equal.astype(np.uint8))
    leaked = privacy.leaked_bits(N, 220, PUNCT.size, SHORT.size, res.disclosed)
    assert np.array_equal(leaked, 160 + res.disclosed) and set(np.unique(res.disclosed)) == {0, STEP}
    lengths = privacy.secret_length(n_key, leaked, QBER, 64, 30)
    lengths[ok == 0] = 0
    assert set(np.unique(lengths[lengths > 0])) == {592, 572}, "round 0 and round 1 frames differ by the disclosed bits"
    pa_seed = rng.integers(0, 2, n_key + int(lengths.max()) - 1).astype(np.uint8)
    out_a, len_a = privacy.amplify(key_a, pa_seed, lengths)
    out_b, len_b = privacy.amplify(key_b, pa_seed, lengths)
    assert np.array_equal(len_a, lengths) and np.array_equal(len_b, lengths)
    assert np.array_equal(out_a[ok == 1], out_b[ok == 1]) and out_a[ok == 1].any()
