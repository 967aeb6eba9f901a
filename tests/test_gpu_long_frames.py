"""The two-party, blind, select and estimate entries on frames long enough for
1024 threads per frame, and on split frames.

Every one-workgroup-per-frame kernel of parties.hip, blind.hip, select.hip and
estimate.hip launches aux_frame_threads(n) threads: 256 below n = 32768, 1024
from there up.  The graphs here:
  - shape_codes.long_split (n = 33001, odd; 2 parts of 16 waves): the smallest
    shape with 1024 threads per frame and a split decode.  The odd n leaves a
    partial last key word, wave ballot and 4-codes-per-byte group;
  - regular codes of n = 32767 and n = 32768, the two sides of the threshold,
    for the kernels that need no decode (the same inputs and checks, another
    launch width);
  - the committed C4 stand-in (n = 102400) where n itself matters: a select
    whose dynamic LDS goes beyond 64 KB, and one short chain end to end.

The checkers are numpy (symmetric_ref, estimate_ref, test_gpu_parties'
np_extend / np_llr) and the CPU oracle; everything is compared bit for bit.

Frames: Q.bsc_frames one frame at a time, frame f at QBER q0 (1 + 0.04 (f -
3.5)) with its own log_p, so that a batch of 8 straddles the waterfall of a
12-iteration decode whatever the noise draws; q0 per algorithm and plan was
chosen with the oracle alone (Q0 below, the oracle's counts beside it), and
every non-degeneracy condition is asserted on the oracle's own results.

Not covered here: bob_frames_kernel's col_orig arm.  Only unsplit graphs
without scratch slots are relabelled (layout.hip relabel()), every graph of
n >= 32768 is split, and so col_orig is NULL on all of these graphs;
test_gpu_parties.test_relabelled_graph (C2) is the test of that arm.
"""
import functools

import numpy as np
import pytest

import estimate_ref as R
import qkd_ldpc_v_amd as Q
import shape_codes as S
from conftest import bits_equal_nan, diag_env, load_fixture
from oracle.pyoracle import Oracle
from symmetric_ref import np_symmetric
from test_gpu_blind import device_round, merged, pinned_llr
from test_gpu_estimate import device_errors, device_estimate
from test_gpu_parties import RA_ALGS, alice_device, assert_mixed, assert_same, bob_device, cuda, np_extend, np_llr
from test_gpu_symmetric import (FILL, LISTED, assert_exchange, device_positions_round, device_select, histories,
                                np_positions, synthetic_posteriors)

pytestmark = pytest.mark.gpu

C4S = "c4s_n102400_m32001.alist"
LS_N = 33001
THRESHOLD = {32767: 6553, 32768: 6554}  # n -> m of the regular codes on the two sides of aux_frame_threads' step
BATCH, CAP, LADDER = 8, 12, 0.04
N_PUNCT, N_SHORT = 1500, 300
SPA, OMSA, AOMSA = RA_ALGS
ROUND_ALGS = [SPA, OMSA]
PAD = 64  # sentinel bytes after an output
C4_LISTS = (40, 10, 9)  # the C4 stand-in's small plan: plan_lists' n_punct, n_short, seed

# (algorithm, with the plan) -> q0.  The oracle at cap 12, 8 frames: converged after >= 2 iterations / at the cap
Q0 = {
    (Q.SPA, True): 0.0110, (Q.SPA, False): 0.0165,     # 5/3, 5/3 (at 0.0103: 8/0; at 0.0175: 1/7)
    (Q.OMSA, True): 0.0090, (Q.OMSA, False): 0.0130,   # 5/3, 4/4
    (Q.AOMSA, True): 0.0097, (Q.AOMSA, False): 0.0142,  # 3/5, 4/4
}
# Frames failing after rounds 0 / 1 / 2 of the oracle.  Fixed order, 200 punctured bits per round: SPA 3/2/0,
# OMSA 3/2/1 (100: 3/2/2, 3/3/2; 300: 3/1/0; 500: 3/0).  Symmetric, 16 positions per round: with the plan SPA
# 3/1/0, OMSA 3/1/0; without 3/2/1, 4/2/1 (40 and more: nothing fails round 1; 4: nothing newly decodes in it)
BLIND_STEP = 200
SYM_STEP = 16


# ---- the graphs ------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def matrix(n):
    if n == LS_N:
        return S.long_split()
    if n in THRESHOLD:
        return Q.regular_code(n, THRESHOLD[n], 3, 1)
    assert n == 102400
    return load_fixture(C4S)


@functools.lru_cache(maxsize=None)
def graphs(n):
    """(Alice's, Bob's) device graphs.  The threshold pair and the C4 stand-in
    serve both sides with one graph: no test here decodes on the former, and
    the latter is the costliest graph of the suite to create."""
    ga = Q.Graph(matrix(n))
    return ga, (Q.Graph(matrix(n)) if n == LS_N else ga)


@functools.lru_cache(maxsize=None)
def oracle(n):
    return Oracle(matrix(n))


@functools.lru_cache(maxsize=None)
def plan_lists(n, n_punct=N_PUNCT, n_short=N_SHORT, seed=5):
    """(punctured, shortened), ascending: the first and last positions and both
    sides of the word, wave and workgroup boundaries (0, 31, 32, 63, 64, 1023,
    1024, 32767, 32768, n - 1 where they exist) dealt alternately to the two
    lists, the rest drawn."""
    edges = [e for e in (0, 31, 32, 63, 64, 1023, 1024, 32767, 32768) if e < n - 1] + [n - 1]
    pe, se = edges[0::2], edges[1::2]
    rest = np.random.Generator(np.random.PCG64(seed)).permutation(np.setdiff1d(np.arange(n), edges))
    punct = np.sort(np.concatenate([pe, rest[:n_punct - len(pe)]])).astype(np.int32)
    short = np.sort(np.concatenate([se, rest[n_punct:n_punct + n_short - len(se)]])).astype(np.int32)
    assert punct.size == n_punct and short.size == n_short and np.intersect1d(punct, short).size == 0
    assert np.isin(edges, np.concatenate([punct, short])).all()
    for a in (punct, short):
        a.setflags(write=False)
    return punct, short


def keypos(n, punct, short):
    return np.setdiff1d(np.arange(n), np.concatenate([punct, short]))


# ---- the frames and the oracle's side ---------------------------------------------------
@functools.lru_cache(maxsize=None)
def frames(n, q0, with_plan, batch=BATCH, seed=40, lists=()):
    """-> alice, bob, fill, log_p [batch], ext, syndrome, llr0 (fill: None
    without the plan; lists: plan_lists' arguments after n)."""
    H = matrix(n)
    rows = [Q.bsc_frames(n, q0 * (1.0 + LADDER * (f - (batch - 1) / 2)), 1, seed=seed + f) for f in range(batch)]
    a, b = np.concatenate([r[0] for r in rows]), np.concatenate([r[1] for r in rows])
    lp = np.array([Q.log_p(r[2]) for r in rows])
    if not with_plan:
        return a, b, None, lp, a, H.syndrome(a), np_llr(b, lp)
    punct, short = plan_lists(n, *lists)
    fill = np.random.Generator(np.random.PCG64(3)).integers(0, 2, (batch, punct.size)).astype(np.uint8)
    ext = np_extend(a, fill, punct, short)
    return a, b, fill, lp, ext, H.syndrome(ext), np_llr(b, lp, punct, short)


def ls_frames(alg, with_plan):
    return frames(LS_N, Q0[alg, with_plan], with_plan)


@functools.lru_cache(maxsize=None)
def ls_round0(alg, prim, sec, with_plan):
    """The oracle's one-shot decode of ls_frames, not degenerate: at least 2
    frames converge after >= 2 iterations and at least 2 reach the cap."""
    *_, syn, llr0 = ls_frames(alg, with_plan)
    O = oracle(LS_N)
    want = O.decode_batch(O.params(alg, CAP, True, 100.0, prim, sec), llr0, syn, threads=16, posterior=True)
    assert_mixed(want, least=2)
    return want


def assert_rounds(states, what):
    """At least 2 frames fail round 0, at least 1 newly decodes in round 1 and at least 1 goes on to round 2."""
    assert len(states) >= 3, (what, len(states))
    ok0, ok1 = states[0][2], states[1][2]
    assert int((ok0 == 0).sum()) >= 2 and int(((ok0 == 0) & (ok1 == 1)).sum()) >= 1 and int((ok1 == 0).sum()) >= 1, \
        (what, ok0, ok1)


@functools.lru_cache(maxsize=None)
def ls_blind(alg, prim, sec):
    """Rounds 0, 1, 2 in ascending order of the punctured list, BLIND_STEP bits per round."""
    _, _, fill, _, _, syn, llr0 = ls_frames(alg, True)
    punct, _ = plan_lists(LS_N)
    O = oracle(LS_N)
    st = ls_round0(alg, prim, sec, True)
    states, lists = [st], []
    for r in (1, 2):
        failed = np.flatnonzero(st[2] == 0)
        if failed.size == 0:
            break
        res = O.decode_batch(O.params(alg, CAP, True, 100.0, prim, sec),
                             pinned_llr(llr0, punct, fill, failed, np.arange(BLIND_STEP * r)), syn[failed], threads=16,
                             posterior=True)
        st = merged(st, failed, res)
        states.append(st)
        lists.append(failed)
    assert_rounds(states, ("blind", alg))
    return states, lists


@functools.lru_cache(maxsize=None)
def ls_symmetric(alg, prim, sec, with_plan):
    _, _, _, _, ext, syn, llr0 = ls_frames(alg, with_plan)
    short = plan_lists(LS_N)[1] if with_plan else None
    O = oracle(LS_N)
    res = np_symmetric(O, O.params(alg, CAP, True, 100.0, prim, sec), llr0, syn, ext, short, SYM_STEP, 2)
    assert_rounds(res[0], ("symmetric", alg, with_plan))
    assert all(np.array_equal(x, y) for x, y in zip(res[0][0][:3], ls_round0(alg, prim, sec, with_plan)[:3]))
    return res


# ---- 1. Alice ----------------------------------------------------------------------------
def alice_padded(g, alice, plan=None, fill=None):
    """alice_device on outputs followed by PAD sentinel bytes, which must stay."""
    import torch

    batch = alice.shape[0]
    syn = torch.full((batch * g.m + PAD,), 7, dtype=torch.uint8, device="cuda")
    ext = torch.full((batch * g.n + PAD,), 7, dtype=torch.uint8, device="cuda") if plan is not None else None
    g.syndrome_device(cuda(alice), syn, plan, None if fill is None else cuda(fill), ext)
    torch.cuda.synchronize()
    hs = syn.cpu().numpy()
    assert (hs[batch * g.m:] == 7).all(), "the syndrome was written past its end"
    if ext is None:
        return hs[:batch * g.m].reshape(batch, g.m), None
    hx = ext.cpu().numpy()
    assert (hx[batch * g.n:] == 7).all(), "the extended key was written past its end"
    return hs[:batch * g.m].reshape(batch, g.m), hx[:batch * g.n].reshape(batch, g.n)


def check_alice(n, case):
    H = matrix(n)
    ga, _ = graphs(n)
    rng = np.random.Generator(np.random.PCG64(n))
    alice = rng.integers(0, 2, (5, n), dtype=np.uint8)
    high = 0xFE if case == "high bits" else 0
    if case == "no plan":
        syn, ext = alice_padded(ga, alice)
        assert ext is None and np.array_equal(syn, H.syndrome(alice)), "Alice's syndrome differs from H * alice"
        return
    punct, short = plan_lists(n)
    fill = rng.integers(0, 2, (5, punct.size), dtype=np.uint8)
    want_ext = np_extend(alice, fill, punct, short)
    syn, ext = alice_padded(ga, alice | high, ga.rate_plan(punct, short), fill | high)  # (only bit 0 counts)
    assert np.array_equal(ext, want_ext), "the extended key differs from numpy's"
    assert np.array_equal(syn, H.syndrome(want_ext)), "the syndrome differs from H * the extended key"


@pytest.mark.parametrize("case", ["plan", "no plan", "high bits"])
def test_alice_on_split_frames(gpu_available, case):
    check_alice(LS_N, case)
    assert graphs(LS_N)[0].split_plan()["parts"] > 1
    S.assert_plan(graphs(LS_N)[0], "long_split")


@pytest.mark.parametrize("case", ["plan", "no plan", "high bits"])
@pytest.mark.parametrize("n", list(THRESHOLD))
def test_alice_at_the_width_threshold(gpu_available, n, case):
    check_alice(n, case)


# ---- 2. Bob's reconcile on split frames ---------------------------------------------------
@pytest.mark.parametrize("with_plan", [True, False], ids=["plan", "no plan"])
@pytest.mark.parametrize("alg,prim,sec", RA_ALGS)
def test_bob_reconcile_on_split_frames(gpu_available, alg, prim, sec, with_plan):
    _, gb = graphs(LS_N)
    _, bob, _, lp, _, syn, llr0 = ls_frames(alg, with_plan)
    want = ls_round0(alg, prim, sec, with_plan)
    plan = gb.rate_plan(*plan_lists(LS_N)) if with_plan else None
    par = Q.Params(alg, CAP, True, 100.0, prim, sec)
    out, _ = bob_device(gb, par, bob, lp, syn, plan=plan)
    assert_same(out, want, "reconcile on split frames (no LLR workspace)")
    if alg == Q.SPA:  # the f64 arm and the codes arm of bob_frames_kernel in one call
        out, ws = bob_device(gb, par, bob, lp, syn, plan=plan, llr_ws=True)
        assert bits_equal_nan(ws, llr0), "Bob's LLR workspace differs from numpy's"
        assert_same(out, want, "reconcile on split frames (LLR workspace given)")
    assert gb.split_plan()["parts"] > 1
    S.assert_plan(gb, "long_split", alg)


@pytest.mark.parametrize("layout", ["frame_per_lane", "v1"])
def test_bob_reconcile_layouts_that_read_the_llrs(gpu_available, layout):
    H = matrix(LS_N)
    alg, prim, sec = SPA
    if layout == "v1":
        with diag_env(QLDPC_VARIANT="v1"):  # (read at graph creation)
            g = Q.Graph(H)
        assert g.plan(0, alg)["variant"] == "glb_glb"  # (99,003 edges: messages and totals in global memory)
    else:
        g = Q.Graph(H, layout=layout)
        assert g.plan(0, alg)["variant"] == "fpl"
    _, bob, _, lp, _, syn, _ = ls_frames(alg, True)
    out, _ = bob_device(g, Q.Params(alg, CAP, True, 100.0, prim, sec), bob, lp, syn, plan=g.rate_plan(*plan_lists(LS_N)))
    assert_same(out, ls_round0(alg, prim, sec, True), layout)


# ---- 3. key extraction, corrected errors, syndrome weight under a plan ------------------------
def device_key(g, plan, bits):
    import torch

    batch = bits.shape[0]
    key = torch.full((batch * plan.n_key + PAD,), 7, dtype=torch.uint8, device="cuda")
    g.extract_key_device(plan, cuda(bits), key)
    torch.cuda.synchronize()
    h = key.cpu().numpy()
    assert (h[batch * plan.n_key:] == 7).all(), "the key was written past its end"
    return h[:batch * plan.n_key].reshape(batch, plan.n_key)


def check_key_errors_weight(n, g, bob, bits, syn):
    """extract_key_device against the inverse of the extension, corrected_errors
    and the syndrome weight under the plan against estimate_ref."""
    H = matrix(n)
    punct, short = plan_lists(n)
    plan = g.rate_plan(punct, short)
    kp = keypos(n, punct, short)
    assert plan.n_key == kp.size == n - N_PUNCT - N_SHORT
    assert np.array_equal(device_key(g, plan, bits), bits[:, kp]), "extract_key differs from bits at the key positions"
    want = R.corrected_errors(bob, bits, punct, short)
    assert np.unique(want).size > 1
    assert np.array_equal(device_errors(g, bob, bits, plan), want), "corrected errors differ"
    assert np.array_equal(device_errors(g, bob | 0xFE, bits | 0xFE, plan), want), "only bit 0 is read"
    assert np.array_equal(device_errors(g, bob, bits), R.corrected_errors(bob, bits)), "corrected errors (no plan) differ"
    want_w = R.weights_csr(H, bob, syn, punct, short)
    assert np.unique(want_w).size > 1
    got = device_estimate(g, bob, syn, plan, want=("weight",))["weight"]
    assert got.dtype == np.int32 and np.array_equal(got, want_w), "syndrome weights under the plan differ"


def test_key_errors_weight_on_split_frames(gpu_available):
    _, gb = graphs(LS_N)
    alg, prim, sec = SPA
    _, bob, _, _, _, syn, _ = ls_frames(alg, True)
    check_key_errors_weight(LS_N, gb, bob, ls_round0(alg, prim, sec, True)[0], syn)
    assert gb.split_plan()["parts"] > 1


@pytest.mark.parametrize("n", list(THRESHOLD))
def test_key_errors_weight_at_the_width_threshold(gpu_available, n):
    rng = np.random.Generator(np.random.PCG64(n + 1))
    bob = rng.integers(0, 2, (5, n), dtype=np.uint8)
    bits = R.extend(bob, n, *plan_lists(n)) ^ (rng.random((5, n)) < np.linspace(0.0, 0.04, 5)[:, None]).astype(np.uint8)
    syn = rng.integers(0, 2, (5, THRESHOLD[n]), dtype=np.uint8)
    check_key_errors_weight(n, graphs(n)[1], bob, bits, syn)


@pytest.mark.parametrize("with_plan", [True, False], ids=["plan", "no plan"])
@pytest.mark.parametrize("n", list(THRESHOLD))
def test_disclose_positions_at_the_width_threshold(gpu_available, n, with_plan):
    """Alice's answer by position.  disclose_positions_kernel runs 256 threads
    whatever n is (aux_frame_threads is not asked), so the two sizes differ in
    n alone: the same rows and checks, counts on both sides of 256."""
    import torch

    ga, _ = graphs(n)
    plan = ga.rate_plan(*plan_lists(n)) if with_plan else None
    rng = np.random.Generator(np.random.PCG64(n + 2))
    ext = rng.integers(0, 256, (9, n + 24)).astype(np.uint8)  # (bit 0 of a byte counts; the bytes past n are never read)
    pos = histories(9, n, 20 + Q.SELECT_MAX, None, seed=6)
    pos[::2, [3, 300]], pos[1::2, [3, 300]] = [0, n - 1], [n - 1, 0]  # the first and the last position, in every row
    assert int((ext > 1).sum()) > n
    d_ext, d_pos = cuda(ext), cuda(pos)
    for first in (0, 20):
        for count in (1, 255, 256, 257, Q.SELECT_MAX):
            out = torch.full((LISTED.size * count + PAD,), 7, dtype=torch.uint8, device="cuda")
            ga.disclose_positions_device(d_ext, cuda(LISTED), d_pos, first, count, out, plan=plan)
            torch.cuda.synchronize()
            got = out.cpu().numpy()
            want = np.stack([ext[f, pos[f, first:first + count]] & 1 for f in LISTED])
            assert (got[LISTED.size * count:] == 7).all(), "Alice's answer was written past its end"
            assert np.array_equal(got[:LISTED.size * count].reshape(LISTED.size, count), want), (n, first, count)


# ---- 4. fixed-order blind rounds on split frames ------------------------------------------------
@pytest.mark.parametrize("alg,prim,sec", ROUND_ALGS)
def test_blind_rounds_on_split_frames(gpu_available, alg, prim, sec):
    _, gb = graphs(LS_N)
    _, bob, fill, lp, _, syn, _ = ls_frames(alg, True)
    states, lists = ls_blind(alg, prim, sec)
    plan = gb.rate_plan(*plan_lists(LS_N))
    par = Q.Params(alg, CAP, True, 100.0, prim, sec)
    kw = dict(bob=bob, lp=lp, syn=syn, fill=fill)
    scrambled = np.roll(lists[0], 1)[::-1]  # (three failed frames a < b < c as b, a, c: neither ascending nor descending)
    assert lists[0].size > 2 and (np.diff(scrambled) > 0).any() and (np.diff(scrambled) < 0).any()
    # (the whole arrays: the rows that are not listed keep the previous round's contents)
    out = device_round(gb, par, plan, scrambled, np.arange(BLIND_STEP), states[0], **kw)
    assert_same(out, states[1], f"round 1 ({lists[0].size} frames, scrambled list)")
    out = device_round(gb, par, plan, lists[1], np.arange(2 * BLIND_STEP), states[1], **kw)
    assert_same(out, states[2], f"round 2 ({lists[1].size} frames)")
    one = lists[0][-1:]
    out = device_round(gb, par, plan, one, np.arange(BLIND_STEP), states[0], **kw)
    assert_same(out, merged(states[0], one, tuple(x[one] for x in states[1])), "round 1, a list of one frame")
    assert gb.split_plan()["parts"] > 1
    S.assert_plan(gb, "long_split", alg)


# ---- 5. symmetric rounds on split frames ------------------------------------------------------------
def check_symmetric_round(ga, gb, par, plan_a, plan_b, short, fx, ref, r, step, listed=None):
    """Round r of ref on the device: Bob's selection, Alice's answer, Bob's
    round.  listed: the round's failed frames in another order, or some of
    them (the others keep the previous round's rows)."""
    import torch

    _, bob, _, lp, ext, syn, _ = fx
    states, lists, _, _, _, positions = ref
    listed, first = lists[r - 1] if listed is None else listed, step * (r - 1)
    assert np.isin(listed, lists[r - 1]).all()
    got = device_select(gb, plan_b, states[r - 1][3], listed, first, step, positions)
    assert np.array_equal(got, np_positions(states[r - 1][3], listed, first, step, short, positions)), f"round {r}: select"
    assert np.array_equal(got[listed, :first + step], positions[listed, :first + step])
    vals = torch.full((listed.size, step), 7, dtype=torch.uint8, device="cuda")
    ga.disclose_positions_device(cuda(ext), cuda(listed.astype(np.int32)), cuda(got), first, step, vals, plan=plan_a)
    torch.cuda.synchronize()
    want = np.stack([ext[f, positions[f, first:first + step]] & 1 for f in listed])
    assert np.array_equal(vals.cpu().numpy(), want), f"round {r}: Alice's answer"
    out = device_positions_round(gb, par, plan_b, listed, first + step, positions, ext, states[r - 1], bob, lp, syn)
    want = merged(states[r - 1], listed, tuple(x[listed] for x in states[r]))
    assert_same(out, want, f"round {r} (frames {listed.tolist()})")  # listed and unlisted rows alike


@pytest.mark.parametrize("with_plan", [True, False], ids=["plan", "no plan"])
@pytest.mark.parametrize("alg,prim,sec", ROUND_ALGS)
def test_symmetric_rounds_on_split_frames(gpu_available, alg, prim, sec, with_plan):
    ga, gb = graphs(LS_N)
    ref = ls_symmetric(alg, prim, sec, with_plan)
    lists = plan_lists(LS_N) if with_plan else None
    plan_a, plan_b = (ga.rate_plan(*lists), gb.rate_plan(*lists)) if with_plan else (None, None)
    par = Q.Params(alg, CAP, True, 100.0, prim, sec)
    args = (ga, gb, par, plan_a, plan_b, lists[1] if with_plan else None, ls_frames(alg, with_plan), ref)
    # round 1 as test 4 gives it: the list scrambled (b, a, c ...: list[j] is no row index of the compact decode,
    # neither ascending nor descending), then whole, then its last frame alone
    failed = ref[1][0]
    scrambled = np.roll(failed, 1)[::-1]
    assert failed.size > 2 and (np.diff(scrambled) > 0).any() and (np.diff(scrambled) < 0).any()
    check_symmetric_round(*args, 1, SYM_STEP, listed=scrambled)
    check_symmetric_round(*args, 1, SYM_STEP, listed=failed[-1:])
    for r in (1, 2):
        check_symmetric_round(*args, r, SYM_STEP)
    assert gb.split_plan()["parts"] > 1
    S.assert_plan(gb, "long_split", alg)


def test_symmetric_reconcile_on_split_frames(gpu_available):
    ga, gb = graphs(LS_N)
    alg, prim, sec = SPA
    alice, bob, fill, lp, ext, _, _ = ls_frames(alg, True)
    lists = plan_lists(LS_N)
    ref = ls_symmetric(alg, prim, sec, True)
    res = Q.symmetric_reconcile(ga, ga.rate_plan(*lists), gb, gb.rate_plan(*lists),
                                Q.Params(alg, CAP, True, 100.0, prim, sec), alice, bob, lp, fill, SYM_STEP, max_rounds=2)
    assert_exchange(res, ref, ext)
    assert res.rounds.max() == 2 and res.positions.shape == (BATCH, 2 * SYM_STEP)


# ---- 6. the select at width 1024 ---------------------------------------------------------------------
COUNTS = (1, 63, 64, 65, 1023, 1024, 1025, 4095, 4096)


def select_setup(n, with_plan):
    _, g = graphs(n)
    if not with_plan:
        return g, None, None
    punct, short = plan_lists(n, *C4_LISTS) if n == 102400 else plan_lists(n)
    return g, g.rate_plan(punct, short), short


@pytest.mark.parametrize("with_plan", [True, False], ids=["plan", "no plan"])
@pytest.mark.parametrize("first", [0, 20])
@pytest.mark.parametrize("n", [LS_N] + list(THRESHOLD))
def test_select_against_numpy(gpu_available, n, first, with_plan):
    """1024 threads: 2 histogram bins per thread (1 in the last digit, behind
    `tid * per < bins`), 16 waves in block_scan, counts up to QLDPC_SELECT_MAX."""
    g, plan, short = select_setup(n, with_plan)
    post = synthetic_posteriors(n)
    hist = histories(9, n, first + Q.SELECT_MAX, short)
    got = {}
    for count in COUNTS:
        got[count] = device_select(g, plan, post, LISTED, first, count, hist)
        want = np_positions(post, LISTED, first, count, short, hist)
        bad = np.flatnonzero((got[count] != want).any(axis=1))
        # (the whole array: unlisted rows and the columns outside [first, first + count) keep FILL)
        assert bad.size == 0, f"n {n}, count {count}, first {first}: rows {bad.tolist()} differ"
    for count in COUNTS[:-1]:
        assert np.array_equal(got[count][:, :first + count], got[4096][:, :first + count]), "a shorter selection is a prefix"
    if with_plan:
        assert not np.isin(got[4096][LISTED, first:], short).any(), "a shortened position was chosen"


@pytest.mark.parametrize("n", [LS_N] + list(THRESHOLD))
def test_select_in_two_calls(gpu_available, n):
    """QLDPC_SELECT_MAX positions, then as many again with the first call's as history: numpy's 8192, in order."""
    g, plan, short = select_setup(n, True)
    post = synthetic_posteriors(n)
    none = np.full((9, 2 * Q.SELECT_MAX), FILL, np.int32)
    one = device_select(g, plan, post, LISTED, 0, Q.SELECT_MAX, none)
    two = device_select(g, plan, post, LISTED, Q.SELECT_MAX, Q.SELECT_MAX, one)
    assert np.array_equal(two, np_positions(post, LISTED, 0, 2 * Q.SELECT_MAX, short, none))


def test_select_beyond_64k_of_lds(gpu_available):
    """n = 102400 with count >= 2049: select_lds is 70,224 bytes, past the 64 KB a kernel gets without asking."""
    rows = np.array([5, 0, 3], np.int32)  # one value everywhere, massive ties, specials and NaNs
    post = synthetic_posteriors(102400)
    g, plan, short = select_setup(102400, True)
    hist = histories(9, 102400, 20 + Q.SELECT_MAX, short)
    for count in (4095, 4096):
        got = device_select(g, plan, post, rows, 20, count, hist)
        assert np.array_equal(got, np_positions(post, rows, 20, count, short, hist)), count
    none = np.full((9, 2 * Q.SELECT_MAX), FILL, np.int32)
    one = device_select(g, None, post, rows, 0, Q.SELECT_MAX, none)
    two = device_select(g, None, post, rows, Q.SELECT_MAX, Q.SELECT_MAX, one)
    assert np.array_equal(two, np_positions(post, rows, 0, 2 * Q.SELECT_MAX, None, none))
    assert g.split_plan()["parts"] > 1


# ---- 7. the chain on the C4 stand-in itself ------------------------------------------------------------
# the oracle: frames 1 and 2 fail one-shot and decode in the round (at 0.025: frame 2 alone; at 0.028: all three fail)
C4_Q0, C4_CAP, C4_STEP = 0.026, 8, 400


def test_chain_on_the_c4_stand_in(gpu_available):
    """3 frames, 40 punctured and 10 shortened positions: Alice's syndrome, Bob's
    reconcile (SPA, 8 iterations), one symmetric round over the frames that
    failed, the key."""
    n = 102400
    H = matrix(n)
    ga, gb = graphs(n)
    punct, short = plan_lists(n, *C4_LISTS)
    plan = gb.rate_plan(punct, short)
    fx = alice, bob, fill, lp, ext, syn, llr0 = frames(n, C4_Q0, True, batch=3, lists=C4_LISTS)
    got_syn, got_ext = alice_device(ga, alice, plan, fill)
    assert np.array_equal(got_ext, ext) and np.array_equal(got_syn, syn)
    O = oracle(n)
    ref = np_symmetric(O, O.params(Q.SPA, C4_CAP, True, 100.0), llr0, syn, ext, short, C4_STEP, 1)
    states, listed = ref[0], ref[1]
    failed0, failed1 = int((states[0][2] == 0).sum()), int((states[1][2] == 0).sum())
    assert 1 <= failed0 <= 2 and failed1 < failed0, (states[0][1], states[0][2], states[1][2])
    par = Q.Params(Q.SPA, C4_CAP, True, 100.0)
    out, _ = bob_device(gb, par, bob, lp, got_syn, plan=plan)
    assert_same(out, states[0], "reconcile on the C4 stand-in")
    check_symmetric_round(ga, gb, par, plan, plan, short, fx, ref, 1, C4_STEP)
    kp = keypos(n, punct, short)
    key = device_key(gb, plan, states[1][0])
    assert np.array_equal(key, states[1][0][:, kp])
    done = states[1][2] == 1
    assert np.array_equal(key[done], alice[done][:, :kp.size]), "a decoded frame's key is not Alice's"
    assert gb.split_plan()["parts"] > 1
