"""Two-party reconciliation on the GPU: Alice's syndromes (qldpc_syndrome_batch*),
Bob's decode from his own key (qldpc_reconcile_batch*) and the key extraction
of rate-adapted frames (qldpc_extract_key_device).

The checker is always the CPU oracle, with numpy for syndromes, the extended
key and Bob's LLRs; equality with the fused entries (which hold both keys) is
asserted in addition.  Alice and Bob use separate Graph objects, and the
syndrome travels between them through host numpy."""
import functools
import sys

import numpy as np
import pytest

import qkd_ldpc_v_amd as Q
from conftest import bits_equal_nan, diag_env, load_fixture
from oracle import pyoracle as P
from oracle.pyoracle import Oracle
from test_gpu_parity import ALGS
from test_rate_adapt import POINTS, SEED, untp

pytestmark = pytest.mark.gpu

C1, C2, C5 = "c1_n1024_m220.alist", "c2_n10240_m2201.alist", "c5_n10240_m2048.sp2"
DBL_MAX = sys.float_info.max
PUNCT = np.array([0, 5, 31, 32, 1023], np.int32)  # first and last positions, both sides of word boundaries
SHORT = np.array([1, 63, 64, 1000], np.int32)
RA_ALGS = [(Q.SPA, 0.0, 0.0), (Q.OMSA, 0.77, 0.0), (Q.AOMSA, 0.55, 1.2)]


# ---- numpy's side: the extension, Bob's LLRs -------------------------------------
def np_extend(alice, fill, punct, short):
    """The extended key (src/qkd_ldpc_algorithm.cpp:1141-1180): key bits in
    order at the key positions, the fill at punctured ones, 0 at shortened."""
    batch, n = alice.shape
    keypos = np.setdiff1d(np.arange(n), np.concatenate([punct, short]))
    ext = np.zeros((batch, n), np.uint8)
    ext[:, keypos] = alice[:, :keypos.size]
    ext[:, punct] = fill
    return ext


def np_llr(bob, lp, punct=None, short=None):
    batch, n = bob.shape
    lp = np.broadcast_to(np.asarray(lp, np.float64), (batch,))[:, None]
    if punct is None:
        return np.where(bob != 0, -lp, lp)
    keypos = np.setdiff1d(np.arange(n), np.concatenate([punct, short]))
    llr = np.empty((batch, n), np.float64)
    llr[:, keypos] = np.where(bob[:, :keypos.size] != 0, -lp, lp)
    llr[:, punct] = 1e-4
    llr[:, short] = DBL_MAX
    return llr


# ---- the two parties on the device -------------------------------------------------
def cuda(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def alice_device(g, alice, plan=None, fill=None):
    """-> (syndrome, extended key or None) as host arrays."""
    import torch

    batch = alice.shape[0]
    syn = torch.full((batch, g.m), 7, dtype=torch.uint8, device="cuda")
    ext = torch.full((batch, g.n), 7, dtype=torch.uint8, device="cuda") if plan is not None else None
    g.syndrome_device(cuda(alice), syn, plan, None if fill is None else cuda(fill), ext)
    torch.cuda.synchronize()
    return syn.cpu().numpy(), None if ext is None else ext.cpu().numpy()


def bob_device(g, par, bob, lp, synd, plan=None, llr_ws=False):
    """-> (DecodeOutput, the LLR workspace or None); asserts the received
    syndrome is still what was passed."""
    import torch

    batch = bob.shape[0]
    d_syn = cuda(synd)
    bits = torch.empty((batch, g.n), dtype=torch.uint8, device="cuda")
    it = torch.empty(batch, dtype=torch.int32, device="cuda")
    ok = torch.empty(batch, dtype=torch.uint8, device="cuda")
    post = torch.empty((batch, g.n), dtype=torch.float64, device="cuda")
    ws = torch.full((batch, g.n), np.nan, dtype=torch.float64, device="cuda") if llr_ws else None
    d_lp = cuda(np.array(np.broadcast_to(np.asarray(lp, np.float64), (batch,))))  # (a writable copy)
    g.reconcile_device(par, cuda(bob), d_lp, d_syn, bits, it, ok, plan=plan, llr_ws=ws, posterior=post)
    torch.cuda.synchronize()
    assert np.array_equal(d_syn.cpu().numpy(), synd), "the received syndrome was written to"
    out = Q.DecodeOutput(bits.cpu().numpy(), it.cpu().numpy().astype(np.uint32), ok.cpu().numpy(), post.cpu().numpy())
    return out, None if ws is None else ws.cpu().numpy()


def assert_same(out, want, what):
    """out: DecodeOutput; want: (bits, iterations, synd_ok, posterior or None)."""
    wb, wi, wk, wp = want
    assert np.array_equal(out.bits, wb), f"{what}: hard bits differ in {int((out.bits != wb).any(axis=1).sum())} frames"
    assert np.array_equal(out.iterations, wi), f"{what}: iterations differ"
    assert np.array_equal(out.synd_ok, wk), f"{what}: syndromes_match differs"
    if wp is not None:
        assert bits_equal_nan(out.posterior, wp), f"{what}: posterior LLRs differ"


def assert_mixed(oracle_out, least=5):
    """The batch is not degenerate: frames that converge after >= 2 iterations
    and frames that reach the cap, at least `least` of each."""
    _, it, ok, _ = oracle_out
    assert int(((ok == 1) & (it >= 2)).sum()) >= least and int((ok == 0).sum()) >= least, (it, ok)


@functools.lru_cache(maxsize=None)
def c1_graphs():
    H = load_fixture(C1)
    return Q.Graph(H), Q.Graph(H)  # Alice's, Bob's


@functools.lru_cache(maxsize=None)
def c1_frames():
    H = load_fixture(C1)
    a, b, q = Q.bsc_frames(H.n, 0.02, 70, seed=7)
    lp = Q.log_p(q)
    return a, b, lp, np_llr(b, lp), H.syndrome(a)


@functools.lru_cache(maxsize=None)
def c1_oracle(alg, prim, sec, cap=20):
    H = load_fixture(C1)
    _, _, _, llr, syn = c1_frames()
    O = Oracle(H)
    return O.decode_batch(O.params(alg, cap, True, 100.0, prim, sec), llr, syn, threads=8, posterior=True)


# ---- 1. plain frames on the register kernel, every algorithm ----------------------
@pytest.mark.parametrize("alg,prim,sec", ALGS)
def test_plain_frames_every_algorithm(gpu_available, alg, prim, sec):
    import torch

    H = load_fixture(C1)
    ga, gb = c1_graphs()
    assert ga is not gb and gb.plan(0, alg)["variant"] == "v2"
    alice, bob, lp, llr, syn = c1_frames()
    want = c1_oracle(alg, prim, sec)
    assert_mixed(want)
    par = Q.Params(alg, 20, True, 100.0, prim, sec)

    got_syn, _ = alice_device(ga, alice)
    assert np.array_equal(got_syn, syn), "Alice's syndrome differs from H * alice"
    out, ws = bob_device(gb, par, bob, lp, got_syn, llr_ws=True)
    assert bits_equal_nan(ws, llr), "Bob's LLR workspace differs from numpy's"
    assert_same(out, want, "reconcile (LLR workspace given)")
    out, _ = bob_device(gb, par, bob, lp, got_syn)
    assert_same(out, want, "reconcile (no LLR workspace)")

    # the fused entry on the same keys
    batch = alice.shape[0]
    fs = torch.empty((batch, H.m), dtype=torch.uint8, device="cuda")
    fb = torch.empty((batch, H.n), dtype=torch.uint8, device="cuda")
    fi = torch.empty(batch, dtype=torch.int32, device="cuda")
    fo = torch.empty(batch, dtype=torch.uint8, device="cuda")
    fk = torch.empty(batch, dtype=torch.uint8, device="cuda")
    gb.qkd_ldpc_device(par, cuda(alice), cuda(bob), cuda(np.full(batch, lp)), None, fs, fb, fi, fo, fk)
    torch.cuda.synchronize()
    assert np.array_equal(fs.cpu().numpy(), got_syn)
    fused = (fb.cpu().numpy(), fi.cpu().numpy().astype(np.uint32), fo.cpu().numpy(), None)
    assert_same(out, fused, "reconcile vs the fused entry")


# ---- 2. the layouts that read llr[] ----------------------------------------------
@pytest.mark.parametrize("layout", ["frame_per_lane", "v1"])
@pytest.mark.parametrize("alg,prim,sec", [ALGS[0], ALGS[5]])
def test_other_layouts(gpu_available, layout, alg, prim, sec):
    H = load_fixture(C1)
    if layout == "v1":
        with diag_env(QLDPC_VARIANT="v1"):  # (read at graph creation)
            gb = Q.Graph(H)
        assert gb.plan(0, alg)["variant"] == "reg_lds"
    else:
        gb = Q.Graph(H, layout=layout)  # 70 frames: a full tile of 64 and a partial one
        assert gb.plan(0, alg)["variant"] == "fpl"
    alice, bob, lp, llr, syn = c1_frames()
    got_syn, _ = alice_device(gb, alice)
    assert np.array_equal(got_syn, syn)
    out, _ = bob_device(gb, Q.Params(alg, 20, True, 100.0, prim, sec), bob, lp, syn)  # d_llr_ws = None
    assert_same(out, c1_oracle(alg, prim, sec), layout)


# ---- 3. relabelled 1024-lane graph: the codes go through col_orig ------------------
def test_relabelled_graph(gpu_available):
    H = load_fixture(C2)
    ga, gb = Q.Graph(H), Q.Graph(H)
    lab, _ = gb.labels()
    assert not np.array_equal(lab, np.arange(H.n)), "C2 is expected to be relabelled"
    alice, bob, q = Q.bsc_frames(H.n, 0.0215, 8, seed=3)
    lp = Q.log_p(q)
    syn = H.syndrome(alice)
    got_syn, _ = alice_device(ga, alice)
    assert np.array_equal(got_syn, syn)
    O = Oracle(H)
    want = O.decode_batch(O.params(Q.SPA, 5, True, 100.0), np_llr(bob, lp), syn, threads=8, posterior=True)
    out, ws = bob_device(gb, Q.Params(Q.SPA, 5, True, 100.0), bob, lp, got_syn, llr_ws=True)
    assert bits_equal_nan(ws, np_llr(bob, lp))
    assert_same(out, want, "C2")
    out, _ = bob_device(gb, Q.Params(Q.SPA, 5, True, 100.0), bob, lp, got_syn)
    assert_same(out, want, "C2 (no LLR workspace)")


# ---- 4. odd sizes: n < 32, n % 4 != 0, unaligned frame rows ------------------------
@pytest.mark.parametrize("name", ["kat_n6_m4.dense", "u_n7_m3.dense", "u_n10_m5.dense"])
def test_odd_sizes(gpu_available, name):
    H = load_fixture(name)
    g = Q.Graph(H)
    rng = np.random.Generator(np.random.PCG64(17))
    alice = rng.integers(0, 2, (5, H.n), dtype=np.uint8)
    bob = rng.integers(0, 2, (5, H.n), dtype=np.uint8)
    lp = np.array([Q.log_p(q) for q in (0.01, 0.02, 0.05, 0.1, 0.2)])  # one log_p per frame
    syn = H.syndrome(alice)
    got_syn, _ = alice_device(g, alice)
    assert np.array_equal(got_syn, syn)
    O = Oracle(H)
    want = O.decode_batch(O.params(Q.SPA, 3, True, 100.0), np_llr(bob, lp), syn, threads=2, posterior=True)
    out, ws = bob_device(g, Q.Params(Q.SPA, 3, True, 100.0), bob, lp, syn, llr_ws=True)
    assert bits_equal_nan(ws, np_llr(bob, lp))
    assert_same(out, want, name)
    out, _ = bob_device(g, Q.Params(Q.SPA, 3, True, 100.0), bob, lp, syn)
    assert_same(out, want, name + " (no LLR workspace)")


# ---- 5. rate-adapted, hand-made plan ---------------------------------------------
@functools.lru_cache(maxsize=None)
def ra_frames():
    H = load_fixture(C1)
    a, b, q = Q.bsc_frames(H.n, 0.018, 70, seed=11)
    fill = np.random.Generator(np.random.PCG64(3)).integers(0, 2, (70, 5)).astype(np.uint8)
    lp = Q.log_p(q)
    ext = np_extend(a, fill, PUNCT, SHORT)
    return a, b, fill, lp, ext, H.syndrome(ext), np_llr(b, lp, PUNCT, SHORT)


@functools.lru_cache(maxsize=None)
def ra_oracle(alg, prim, sec):
    H = load_fixture(C1)
    *_, syn, llr = ra_frames()
    O = Oracle(H)
    return O.decode_batch(O.params(alg, 20, True, 100.0, prim, sec), llr, syn, threads=8, posterior=True)


def test_rate_adapted_alice(gpu_available):
    """The extended key and its syndrome: numpy's, and the fused builder's for
    the same Alice inputs (whatever Bob holds)."""
    import torch

    H = load_fixture(C1)
    ga, _ = c1_graphs()
    plan = ga.rate_plan(PUNCT, SHORT)
    alice, bob, fill, lp, ext, syn, _ = ra_frames()
    got_syn, got_ext = alice_device(ga, alice, plan, fill)
    assert np.array_equal(got_ext, ext) and np.array_equal(got_syn, syn)
    batch = alice.shape[0]
    fx = torch.empty((batch, H.n), dtype=torch.uint8, device="cuda")
    fl = torch.empty((batch, H.n), dtype=torch.float64, device="cuda")
    fs = torch.empty((batch, H.m), dtype=torch.uint8, device="cuda")
    ga.build_frames_rate_adapt_device(plan, cuda(alice), cuda(bob), cuda(fill), cuda(fill), cuda(np.full(batch, lp)),
                                      fx, fl, fs)
    torch.cuda.synchronize()
    assert np.array_equal(fx.cpu().numpy(), got_ext) and np.array_equal(fs.cpu().numpy(), got_syn)
    # without the extended-key output: the same syndrome
    syn2 = torch.empty((batch, H.m), dtype=torch.uint8, device="cuda")
    ga.syndrome_device(cuda(alice), syn2, plan, cuda(fill), None)
    torch.cuda.synchronize()
    assert np.array_equal(syn2.cpu().numpy(), syn)
    # extract_key of the extended key is the key
    key = torch.full((batch, plan.n_key), 7, dtype=torch.uint8, device="cuda")
    ga.extract_key_device(plan, cuda(got_ext), key)
    torch.cuda.synchronize()
    assert plan.n_key == H.n - 9 and np.array_equal(key.cpu().numpy(), alice[:, :plan.n_key])


@pytest.mark.parametrize("alg,prim,sec", RA_ALGS)
def test_rate_adapted_bob(gpu_available, alg, prim, sec):
    import torch

    H = load_fixture(C1)
    _, gb = c1_graphs()
    plan = gb.rate_plan(PUNCT, SHORT)
    _, bob, _, lp, _, syn, llr = ra_frames()
    want = ra_oracle(alg, prim, sec)
    assert_mixed(want)
    par = Q.Params(alg, 20, True, 100.0, prim, sec)
    out, ws = bob_device(gb, par, bob, lp, syn, plan=plan, llr_ws=True)
    assert bits_equal_nan(ws, llr), "Bob's LLRs differ from numpy's (+-lp, 1e-4, DBL_MAX)"
    assert_same(out, want, "rate-adapted reconcile")
    out, _ = bob_device(gb, par, bob, lp, syn, plan=plan)
    assert_same(out, want, "rate-adapted reconcile (no LLR workspace)")
    key = torch.full((bob.shape[0], plan.n_key), 7, dtype=torch.uint8, device="cuda")
    gb.extract_key_device(plan, cuda(out.bits), key)
    torch.cuda.synchronize()
    assert np.array_equal(key.cpu().numpy(), np.delete(out.bits, np.union1d(PUNCT, SHORT), axis=1))


def test_empty_plan_is_the_plain_path(gpu_available):
    ga, gb = c1_graphs()
    alice, bob, lp, _, syn = c1_frames()
    got_syn, got_ext = alice_device(ga, alice, ga.rate_plan([], []), None)
    assert np.array_equal(got_syn, syn) and np.array_equal(got_ext, alice)
    alg, prim, sec = ALGS[0]
    out, ws = bob_device(gb, Q.Params(alg, 20, True, 100.0, prim, sec), bob, lp, syn, plan=gb.rate_plan([], []),
                         llr_ws=True)
    assert bits_equal_nan(ws, np_llr(bob, lp))
    assert_same(out, c1_oracle(alg, prim, sec), "empty plan")


# ---- 6. rate-adapted at the workload's code (the hybrid register kernel) -----------
def test_rate_adapted_workload_code(gpu_available):
    import torch

    H = load_fixture(C5)
    ga, gb = Q.Graph(H), Q.Graph(H)
    st = Q.xoshiro_state(SEED)
    O = Oracle(H)
    batch = 16
    seeds = Q.trial_seeds(SEED, batch)
    par = Q.Params(Q.AOMSA, 50, True, 100.0, 0.7, 0.99)
    for q, d, e in POINTS[1:3]:  # (the generator state chains through the points, as in test_rate_adapt)
        pp, sp, _ = Q.adapt_code_rate(H.n, H.m, q, d, e, untp(), st)
        assert pp.size + sp.size > 0
        pa_plan, pb_plan = ga.rate_plan(pp, sp), gb.rate_plan(pp, sp)
        ds = torch.from_numpy(seeds.view(np.int64)).cuda()
        ta = torch.empty((batch, H.n), dtype=torch.uint8, device="cuda")
        tb = torch.empty_like(ta)
        fa = torch.empty((batch, max(1, pp.size)), dtype=torch.uint8, device="cuda")
        fb = torch.empty_like(fa)
        qa = Q.trials_rate_adapt_device(H.n, q, ds, pp.size, ta, tb, fa, fb)
        torch.cuda.synchronize()
        oa, ol = zip(*[P.trial_rate_adapt(H.n, q, int(sd), pp, sp)[:2] for sd in seeds])
        oa, ol = np.stack(oa), np.stack(ol)
        osyn = H.syndrome(oa)
        # Alice: the generator's buffers unchanged ([batch][n] keys, her fill)
        got_syn, got_ext = alice_device(ga, ta.cpu().numpy(), pa_plan, fa.cpu().numpy() if pp.size else None)
        assert np.array_equal(got_ext, oa) and np.array_equal(got_syn, osyn)
        # Bob: his key and the received syndrome alone
        want = O.decode_batch(O.params(Q.AOMSA, 50, True, 100.0, 0.7, 0.99), ol, osyn, threads=8, posterior=True)
        out, ws = bob_device(gb, par, tb.cpu().numpy(), Q.log_p(qa), got_syn, plan=pb_plan, llr_ws=True)
        assert bits_equal_nan(ws, ol)
        assert_same(out, want, f"C5 q={q}")
        out, _ = bob_device(gb, par, tb.cpu().numpy(), Q.log_p(qa), got_syn, plan=pb_plan)
        assert_same(out, want, f"C5 q={q} (no LLR workspace)")


# ---- 7. a syndrome that is not Alice's --------------------------------------------
def test_foreign_syndrome(gpu_available):
    H = load_fixture(C1)
    _, gb = c1_graphs()
    _, bob, lp, llr, syn = c1_frames()
    bad = syn.copy()
    bad[0, 3] ^= 1
    bad[69, H.m - 1] ^= 1
    O = Oracle(H)
    want = O.decode_batch(O.params(Q.SPA, 5, True, 100.0), llr, bad, threads=8, posterior=True)
    out, _ = bob_device(gb, Q.Params(Q.SPA, 5, True, 100.0), bob, lp, bad)
    assert_same(out, want, "altered syndrome")


# ---- 8. host entries: two shards on one GPU ---------------------------------------
@pytest.mark.parametrize("with_plan", [False, True])
def test_host_entries(gpu_available, with_plan):
    H = load_fixture(C1)
    g2 = Q.Graph(H, devices=[0, 0])
    ga, gb = c1_graphs()
    alg, prim, sec = ALGS[0]
    par = Q.Params(alg, 20, True, 100.0, prim, sec)
    if with_plan:
        alice, bob, fill, lp, ext, syn, _ = ra_frames()
        plan2, plana, planb = (g.rate_plan(PUNCT, SHORT) for g in (g2, ga, gb))
        want = ra_oracle(alg, prim, sec)
    else:
        alice, bob, lp, _, syn = c1_frames()
        fill = ext = plan2 = plana = planb = None
        want = c1_oracle(alg, prim, sec)
    for batch in (5, 1, 0):  # uneven shards, an empty shard, nothing
        a, b = alice[:batch], bob[:batch]
        f = None if fill is None else fill[:batch]
        res = g2.syndrome(a, plan2, f)
        hs, hx = (res[1], res[0]) if with_plan else (res, None)
        assert hs.shape == (batch, H.m) and np.array_equal(hs, syn[:batch])
        if with_plan:
            assert np.array_equal(hx, ext[:batch])
            # rows of n_key entries are the same keys
            assert np.array_equal(g2.syndrome(a[:, :plan2.n_key], plan2, f)[1], hs)
        out = g2.reconcile(par, b, lp, hs, plan=plan2, posterior=True)
        assert_same(out, tuple(x[:batch] for x in want), f"host reconcile, batch {batch}")
        assert g2.reconcile(par, b, np.full(batch, lp), hs, plan=plan2).posterior is None
        if batch:
            ds, dx = alice_device(ga, a, plana, f)
            assert np.array_equal(hs, ds) and (not with_plan or np.array_equal(hx, dx))
            dout, _ = bob_device(gb, par, b, lp, ds, plan=planb)
            assert_same(out, (dout.bits, dout.iterations, dout.synd_ok, dout.posterior), "host vs device entries")
