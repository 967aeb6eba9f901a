"""Blind reconciliation on the GPU: the failed-frame list, Alice's disclosure,
Bob's disclosure rounds (qldpc_reconcile_round*) and blind.blind_reconcile.

The checker is the CPU oracle, with numpy for the lists and the pinned LLRs:
for each round numpy builds the LLRs of the frames the ORACLE still fails
(Bob's frame LLRs, +-DBL_MAX at the disclosed punctured positions) and the
oracle decodes them.  The shared fixture is C1 with 60 punctured and 4
shortened positions, 70 frames at QBER 0.016, a cap of 20 iterations and 20
more disclosed bits per round: most frames fail one-shot and nearly all decode
by round 3."""
import functools
import sys

import numpy as np
import pytest

import qkd_ldpc_v_amd as Q
from conftest import bits_equal_nan, diag_env, load_fixture
from oracle.pyoracle import Oracle
from test_gpu_parties import assert_same, c1_graphs, cuda, np_extend, np_llr

pytestmark = pytest.mark.gpu

C1 = "c1_n1024_m220.alist"
DBL_MAX = sys.float_info.max
PUNCT = np.arange(5, 1024, 16)[:60].astype(np.int32)
PUNCT[0], PUNCT[-1] = 0, 1023
PUNCT = np.unique(PUNCT)
SHORT = np.array([1, 63, 64, 1000], np.int32)
BATCH, CAP, STEP, QBER = 70, 20, 20, 0.016
ROUND_ALGS = [(Q.SPA, 0.0, 0.0), (Q.SPA_LIN, 0.0, 0.0), (Q.AOMSA, 0.55, 1.2)]


# ---- the fixture and numpy's / the oracle's side --------------------------------------
@functools.lru_cache(maxsize=None)
def fixture():
    H = load_fixture(C1)
    assert PUNCT.size == 60 and np.intersect1d(PUNCT, SHORT).size == 0
    a, b, q = Q.bsc_frames(H.n, QBER, BATCH, seed=11)
    fill = np.random.Generator(np.random.PCG64(3)).integers(0, 2, (BATCH, 60)).astype(np.uint8)
    lp = Q.log_p(q)
    ext = np_extend(a, fill, PUNCT, SHORT)
    return a, b, fill, lp, ext, H.syndrome(ext), np_llr(b, lp, PUNCT, SHORT)


def pinned_llr(llr0, punct, fill, frames, disc):
    """Bob's LLRs of the listed frames with the punctured indices disc pinned
    at Alice's bits: bit ? -DBL_MAX : +DBL_MAX (the builder's sign)."""
    llr = llr0[frames].copy()
    llr[:, punct[disc]] = np.where(fill[frames][:, disc] & 1, -DBL_MAX, DBL_MAX)
    return llr


def oracle_params(alg, prim, sec, cap=CAP):
    return Oracle.params(alg, cap, True, 100.0, prim, sec)


@functools.lru_cache(maxsize=None)
def c1_oracle():
    return Oracle(load_fixture(C1))


def oracle_round(alg, prim, sec, frames, disc):
    """The oracle's decode of the listed fixture frames in a round that pins disc: compact rows."""
    _, _, fill, _, _, syn, llr0 = fixture()
    frames, disc = np.asarray(frames, np.int64), np.asarray(disc, np.int64)
    return c1_oracle().decode_batch(oracle_params(alg, prim, sec), pinned_llr(llr0, PUNCT, fill, frames, disc),
                                    syn[frames], threads=8, posterior=True)


def merged(prev, frames, res):
    """prev (bits, iterations, ok, posterior) with rows `frames` replaced by the compact rows of res."""
    out = tuple(x.copy() for x in prev)
    for o, r in zip(out, res):
        o[frames] = r
    return out


def np_blind(alg, prim, sec, order, step=STEP, max_rounds=None):
    """The exchange restated with numpy and the oracle -> the states after
    rounds 0, 1, ..., the failed lists of rounds 1, ..., and per frame the
    round, the disclosed count and the summed iterations."""
    _, _, _, _, _, syn, llr0 = fixture()
    st = c1_oracle().decode_batch(oracle_params(alg, prim, sec), llr0, syn, threads=8, posterior=True)
    states, lists = [st], []
    rounds, disclosed = np.zeros(BATCH, np.int32), np.zeros(BATCH, np.int32)
    iters = st[1].astype(np.uint32)
    r = d = 0
    while d < PUNCT.size and (max_rounds is None or r < max_rounds):
        failed = np.flatnonzero(st[2] == 0)
        if failed.size == 0:
            break
        r, d = r + 1, min(d + step, PUNCT.size)
        res = oracle_round(alg, prim, sec, failed, order[:d])
        st = merged(st, failed, res)
        iters[failed] += res[1].astype(np.uint32)
        rounds[failed], disclosed[failed] = r, d
        states.append(st)
        lists.append(failed)
    return states, lists, rounds, disclosed, iters


@functools.lru_cache(maxsize=None)
def oracle_rounds(alg, prim, sec):
    """Rounds 0..3 in ascending order (k = 0..19, 0..39, 0..59), with the
    fixture's non-degeneracy asserted: in each of rounds 0, 1 and 2 at least 2
    frames newly decode and at least 2 still fail."""
    states, lists, *_ = np_blind(alg, prim, sec, np.arange(60))
    assert len(states) == 4, "the fixture is expected to need all three disclosure rounds"
    for r in range(3):
        before = np.ones(BATCH, bool) if r == 0 else states[r - 1][2] == 0
        newly, still = int((before & (states[r][2] == 1)).sum()), int((states[r][2] == 0).sum())
        assert newly >= 2 and still >= 2, (alg, r, newly, still)
    return states, lists


# ---- the device's side ---------------------------------------------------------------
def device_round(g, par, plan, frames, disc, prev, bob=None, lp=None, syn=None, fill=None, posterior=True):
    """One qldpc_reconcile_round_device call on outputs pre-filled with prev
    (bits, iterations, ok, posterior) -> the whole arrays afterwards."""
    import torch

    _, fb, ffill, flp, _, fsyn, _ = fixture()
    bob, syn, fill = (fb if bob is None else bob), (fsyn if syn is None else syn), (ffill if fill is None else fill)
    batch = bob.shape[0]
    lp = np.array(np.broadcast_to(np.asarray(flp if lp is None else lp, np.float64), (batch,)))
    frames, disc = np.asarray(frames, np.int32), np.asarray(disc, np.int32)
    vals = np.ascontiguousarray(fill[frames.astype(np.int64)][:, disc.astype(np.int64)])
    d_syn = cuda(syn)
    bits, ok = cuda(prev[0]), cuda(prev[2])
    it = cuda(prev[1].astype(np.int32))
    post = cuda(prev[3]) if posterior else None
    g.reconcile_round_device(par, cuda(bob), cuda(lp), d_syn, plan, cuda(frames), cuda(disc), cuda(vals), bits, it, ok,
                             posterior=post)
    torch.cuda.synchronize()
    assert np.array_equal(d_syn.cpu().numpy(), syn), "the received syndrome was written to"
    return Q.DecodeOutput(bits.cpu().numpy(), it.cpu().numpy().astype(np.uint32), ok.cpu().numpy(),
                          post.cpu().numpy() if posterior else None)


def check_rounds(g, alg, prim, sec, which):
    states, lists = oracle_rounds(alg, prim, sec)
    plan = g.rate_plan(PUNCT, SHORT)
    par = Q.Params(alg, CAP, True, 100.0, prim, sec)
    for r in which:
        out = device_round(g, par, plan, lists[r - 1], np.arange(STEP * r), states[r - 1])
        assert_same(out, states[r], f"round {r} ({lists[r - 1].size} frames)")  # listed and unlisted rows alike
    return states


# ---- 1. rounds 1, 2, 3 against the oracle, on the register kernel ----------------------
@pytest.mark.parametrize("alg,prim,sec", ROUND_ALGS)
def test_rounds_against_the_oracle(gpu_available, alg, prim, sec):
    _, gb = c1_graphs()
    assert gb.plan(0, alg)["variant"] == "v2"
    states = check_rounds(gb, alg, prim, sec, (1, 2, 3))
    ext = fixture()[4]
    done = states[3][2] == 1
    assert done.sum() >= BATCH - 10 and np.array_equal(states[3][0][done], ext[done]), "a decoded frame is not Alice's"


# ---- 2. the layouts that read llr[] directly: a full tile + a partial one, a partial one ----
@pytest.mark.parametrize("layout", ["frame_per_lane", "v1"])
def test_round_other_layouts(gpu_available, layout):
    H = load_fixture(C1)
    alg, prim, sec = ROUND_ALGS[0]
    if layout == "v1":
        with diag_env(QLDPC_VARIANT="v1"):  # (read at graph creation)
            g = Q.Graph(H)
        assert g.plan(0, alg)["variant"] == "reg_lds"
    else:
        g = Q.Graph(H, layout=layout)
        assert g.plan(0, alg)["variant"] == "fpl"
    _, lists = oracle_rounds(alg, prim, sec)
    assert lists[0].size > 64 > lists[1].size > 0
    check_rounds(g, alg, prim, sec, (1, 2))


# ---- 3. degenerate rounds -------------------------------------------------------------
def test_no_disclosure_is_reconcile(gpu_available):
    """n_disc == 0 over every frame: reconcile_device's outputs byte for byte."""
    import torch

    _, gb = c1_graphs()
    _, bob, _, lp, _, syn, _ = fixture()
    plan = gb.rate_plan(PUNCT, SHORT)
    for alg, prim, sec in ROUND_ALGS[::2]:
        par = Q.Params(alg, CAP, True, 100.0, prim, sec)
        bits = torch.empty((BATCH, gb.n), dtype=torch.uint8, device="cuda")
        it = torch.empty(BATCH, dtype=torch.int32, device="cuda")
        ok = torch.empty(BATCH, dtype=torch.uint8, device="cuda")
        post = torch.empty((BATCH, gb.n), dtype=torch.float64, device="cuda")
        gb.reconcile_device(par, cuda(bob), cuda(np.full(BATCH, lp)), cuda(syn), bits, it, ok, plan=plan, posterior=post)
        torch.cuda.synchronize()
        want = (bits.cpu().numpy(), it.cpu().numpy().astype(np.uint32), ok.cpu().numpy(), post.cpu().numpy())
        assert_same(Q.DecodeOutput(*want), oracle_rounds(alg, prim, sec)[0][0], "reconcile_device")
        junk = (np.full((BATCH, gb.n), 7, np.uint8), np.full(BATCH, 77, np.uint32), np.full(BATCH, 7, np.uint8),
                np.full((BATCH, gb.n), -7.0))
        out = device_round(gb, par, plan, np.arange(BATCH), [], junk)
        assert_same(out, want, "a round without disclosure")


@pytest.mark.parametrize("frames", [[13], [BATCH - 1], []], ids=["one", "last", "none"])
def test_short_lists(gpu_available, frames):
    """One frame, the last frame alone, and no frame: only the listed rows change."""
    _, gb = c1_graphs()
    alg, prim, sec = ROUND_ALGS[0]
    plan = gb.rate_plan(PUNCT, SHORT)
    par = Q.Params(alg, CAP, True, 100.0, prim, sec)
    junk = (np.full((BATCH, gb.n), 7, np.uint8), np.full(BATCH, 77, np.uint32), np.full(BATCH, 7, np.uint8),
            np.full((BATCH, gb.n), -7.0))
    disc = np.arange(40)
    want = merged(junk, np.asarray(frames, np.int64), oracle_round(alg, prim, sec, frames, disc)) if frames else junk
    assert_same(device_round(gb, par, plan, frames, disc, junk), want, f"list {frames}")
    if frames:  # ... and without the posterior
        out = device_round(gb, par, plan, frames, disc, junk, posterior=False)
        assert_same(out, want[:3] + (None,), f"list {frames}, no posterior")


# ---- 4. Alice's disclosure --------------------------------------------------------------
def test_disclose_device(gpu_available):
    import torch

    ga, _ = c1_graphs()
    plan = ga.rate_plan(PUNCT, SHORT)
    fill = fixture()[2]
    d_fill = cuda(fill)
    _, lists = oracle_rounds(*ROUND_ALGS[0])
    perm = np.random.Generator(np.random.PCG64(9)).permutation(60)
    for frames, disc in ((lists[0], np.arange(20)), (lists[1], perm[:33]), (lists[0], np.arange(60)),
                         (lists[1], perm), (np.array([BATCH - 1]), perm[:7]), (np.array([0]), np.array([59]))):
        out = torch.full((len(frames), len(disc)), 7, dtype=torch.uint8, device="cuda")
        ga.disclose_device(plan, cuda(frames.astype(np.int32)), d_fill, cuda(disc.astype(np.int32)), out)
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), fill[frames][:, disc]), (frames, disc)
    # n_list below the list's capacity: the rows past it are not written
    out = torch.full((5, 20), 7, dtype=torch.uint8, device="cuda")
    ga.disclose_device(plan, cuda(lists[0][:5].astype(np.int32)), d_fill, cuda(np.arange(20, dtype=np.int32)), out,
                       n_list=3)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(got[:3], fill[lists[0][:3]][:, :20]) and (got[3:] == 7).all()


# ---- 5. the failed-frame list ---------------------------------------------------------
@pytest.mark.parametrize("batch", [1, 63, 64, 65, 1025, 5000])
def test_failed_frames_list(gpu_available, batch):
    import torch

    g, _ = c1_graphs()
    rng = np.random.Generator(np.random.PCG64(5))
    cases = [np.zeros(batch, np.uint8), np.ones(batch, np.uint8), rng.integers(0, 2, batch).astype(np.uint8),
             (rng.integers(0, 8, batch) * rng.integers(0, 2, batch)).astype(np.uint8)]  # any non-zero byte is a success
    for ok in cases:
        for shift in (0, 3):  # an aligned buffer, and one that starts 3 bytes into it
            buf = torch.zeros(batch + shift, dtype=torch.uint8, device="cuda")
            d_ok = buf[shift:]
            d_ok.copy_(torch.from_numpy(ok))
            lst = torch.full((batch,), -1, dtype=torch.int32, device="cuda")
            cnt = torch.full((1,), -1, dtype=torch.int32, device="cuda")
            g.failed_frames_device(d_ok, lst, cnt)
            torch.cuda.synchronize()
            want = np.flatnonzero(ok == 0)
            count = int(cnt.cpu()[0])
            assert count == want.size, (batch, shift)
            assert np.array_equal(lst.cpu().numpy()[:count], want), (batch, shift)


# ---- 6. an odd size: n < 32, unaligned rows, one log_p per frame ---------------------------
def test_odd_size(gpu_available):
    H = load_fixture("u_n10_m5.dense")
    g = Q.Graph(H)
    punct, short = np.array([0, 9], np.int32), np.array([4], np.int32)
    plan = g.rate_plan(punct, short)
    rng = np.random.Generator(np.random.PCG64(17))
    alice = rng.integers(0, 2, (5, H.n), dtype=np.uint8)
    bob = rng.integers(0, 2, (5, H.n), dtype=np.uint8)
    fill = rng.integers(0, 2, (5, 2), dtype=np.uint8)
    lp = np.array([Q.log_p(q) for q in (0.01, 0.02, 0.05, 0.1, 0.2)])
    syn = H.syndrome(np_extend(alice, fill, punct, short))
    llr0 = np_llr(bob, lp, punct, short)
    O = Oracle(H)
    par = Q.Params(Q.SPA, 3, True, 100.0)
    st = O.decode_batch(O.params(Q.SPA, 3, True, 100.0), llr0, syn, threads=2, posterior=True)
    for frames, disc in ((np.arange(5), np.array([1])), (np.array([1, 3, 4]), np.array([1, 0]))):
        llr = pinned_llr(llr0, punct, fill, frames, disc)
        assert (np.abs(llr[:, punct[disc]]) == DBL_MAX).all() and (llr[:, 4] == DBL_MAX).all()
        res = O.decode_batch(O.params(Q.SPA, 3, True, 100.0), llr, syn[frames], threads=2, posterior=True)
        out = device_round(g, par, plan, frames, disc, st, bob=bob, lp=lp, syn=syn, fill=fill)
        st = merged(st, frames, res)
        assert_same(out, st, f"n = 10, disc {disc.tolist()}")


# ---- 7. host entries: two shards on one GPU ------------------------------------------------
def test_host_entries(gpu_available):
    H = load_fixture(C1)
    g2 = Q.Graph(H, devices=[0, 0])
    _, gb = c1_graphs()
    alg, prim, sec = ROUND_ALGS[0]
    par = Q.Params(alg, CAP, True, 100.0, prim, sec)
    plan2, planb = g2.rate_plan(PUNCT, SHORT), gb.rate_plan(PUNCT, SHORT)
    _, bob, fill, lp, _, syn, _ = fixture()
    states, lists = oracle_rounds(alg, prim, sec)
    disc = np.arange(STEP)
    for size in (5, 1, 0):  # uneven shards, an empty shard, nothing
        frames = lists[0][-size:] if size else lists[0][:0]
        vals = g2.disclose(plan2, frames, fill, disc)
        assert vals.shape == (size, STEP) and np.array_equal(vals, fill[frames][:, disc])
        prev = Q.DecodeOutput(*(x.copy() for x in states[0]))
        out = g2.reconcile_round(par, bob, lp, syn, plan2, frames, disc, vals, out=prev)
        want = merged(states[0], frames, oracle_round(alg, prim, sec, frames, disc)) if size else states[0]
        assert out is prev
        assert_same(out, want, f"host round, {size} frames")
        assert_same(device_round(gb, par, planb, frames, disc, states[0]), want, f"device round, {size} frames")
        nopost = g2.reconcile_round(par, bob, np.full(BATCH, lp), syn, plan2, frames, disc, vals)
        assert nopost.posterior is None and np.array_equal(nopost.bits[frames], want[0][frames])
        assert not np.delete(nopost.bits, frames, axis=0).any()  # (a fresh output: the other rows are zeros)
    with pytest.raises(Q.QLDPCError, match="EINVAL.*twice"):
        g2.disclose(plan2, [3, 3], fill, disc)
    with pytest.raises(Q.QLDPCError, match="EINVAL.*outside"):
        g2.disclose(plan2, [3], fill, [60])


# ---- 8. the whole exchange ---------------------------------------------------------------
@pytest.mark.parametrize("order", ["ascending", "permuted"])
def test_blind_reconcile(gpu_available, order):
    ga, gb = c1_graphs()
    alg, prim, sec = ROUND_ALGS[0]
    alice, bob, fill, lp, ext, _, _ = fixture()
    perm = None if order == "ascending" else np.random.Generator(np.random.PCG64(9)).permutation(60)
    states, lists, rounds, disclosed, iters = np_blind(alg, prim, sec, np.arange(60) if perm is None else perm)
    assert len(lists) >= 2 and rounds.max() == len(lists)
    res = Q.blind_reconcile(ga, ga.rate_plan(PUNCT, SHORT), gb, gb.rate_plan(PUNCT, SHORT),
                            Q.Params(alg, CAP, True, 100.0, prim, sec), alice, bob, lp, fill, STEP, order=perm, q=QBER)
    assert np.array_equal(res.rounds, rounds) and np.array_equal(res.disclosed, disclosed)
    assert np.array_equal(res.synd_ok, states[-1][2]) and np.array_equal(res.bits, states[-1][0])
    assert np.array_equal(res.iterations, iters)
    done = res.synd_ok == 1
    assert np.array_equal(res.bits[done], ext[done])
    assert bits_equal_nan(res.efficiency, Q.blind_efficiency(1024, 220, 60, 4, disclosed, QBER))
    if perm is None:  # one disclosure round only: the frames still failing stop at round 1
        one = Q.blind_reconcile(ga, ga.rate_plan(PUNCT, SHORT), gb, gb.rate_plan(PUNCT, SHORT),
                                Q.Params(alg, CAP, True, 100.0, prim, sec), alice, bob, lp, fill, STEP, max_rounds=1)
        assert np.array_equal(one.synd_ok, states[1][2]) and np.array_equal(one.bits, states[1][0])
        assert one.rounds.max() == 1 and np.isnan(one.efficiency).all()
