"""Error estimation at the reconciliation stage on the GPU: the syndrome
weights, q and log_p before the decode (qldpc_estimate_qber*), the corrected
errors after it (qldpc_corrected_errors*) and estimate.py.

The checker is tests/estimate_ref.py: integers are compared as integers and
doubles bit for bit; the decode that the estimate feeds is checked against the
CPU oracle."""
import functools

import numpy as np
import pytest

import estimate_ref as R
import qkd_ldpc_v_amd as Q
from conftest import load_fixture
from oracle.pyoracle import Oracle
from qkd_ldpc_v_amd import estimate, privacy
from test_estimate_host import BLIND_PUNCT, BLIND_SHORT, c2_plan_lists, u64, u_plans
from test_gpu_blind import CAP, PUNCT, QBER, ROUND_ALGS, SHORT, STEP, fixture
from test_gpu_parties import assert_same, c1_frames, c1_graphs, cuda, np_llr

pytestmark = pytest.mark.gpu

C1, C2, C4S = "c1_n1024_m220.alist", "c2_n10240_m2201.alist", "c4s_n102400_m32001.alist"
Q_MIN, Q_MAX = 1e-4, 0.25
PAD = 8  # output buffers are this much longer than the batch: the tail keeps its sentinel


def device_estimate(g, keys, synd, plan=None, want=("weight", "qber", "log_p"), q_min=Q_MIN, q_max=Q_MAX, d_keys=None,
                    stream=None):
    """-> {name: host array of batch entries}; asserts the sentinels past the batch."""
    import torch

    batch = keys.shape[0] if d_keys is None else d_keys.shape[0]
    bufs = {"weight": torch.full((batch + PAD,), -77, dtype=torch.int32, device="cuda"),
            "qber": torch.full((batch + PAD,), -7.5, dtype=torch.float64, device="cuda"),
            "log_p": torch.full((batch + PAD,), -7.5, dtype=torch.float64, device="cuda")}
    args = {k: (bufs[k] if k in want else None) for k in bufs}
    g.estimate_qber_device(cuda(keys) if d_keys is None else d_keys, cuda(synd), args["weight"], args["qber"],
                           args["log_p"], plan=plan, q_min=q_min, q_max=q_max, stream=stream)
    torch.cuda.synchronize()
    out = {}
    for k, b in bufs.items():
        h = b.cpu().numpy()
        sentinel = -77 if k == "weight" else -7.5
        assert np.all(h[batch:] == sentinel), f"{k}: written past the batch"
        if k in want:
            out[k] = h[:batch]
        else:
            assert np.all(h == sentinel), f"{k}: written though not asked for"
    return out


def check_against_reference(g, H, keys, synd, punct=None, short=None, plan=None, solve=True, csr=False):
    if csr:
        want_w = R.weights_csr(H, keys, synd, punct, short)
    else:
        want_w = R.weights(dense_of(H), keys, synd, punct, short)
    got = device_estimate(g, keys, synd, plan, want=("weight", "qber", "log_p") if solve else ("weight",))
    assert got["weight"].dtype == np.int32 and np.array_equal(got["weight"], want_w), "syndrome weights differ"
    if solve:
        deg, cnt = R.classes(dense_of(H), punct, short)
        want_q = np.array([R.qber(deg, cnt, k, Q_MIN, Q_MAX) for k in want_w])
        assert np.array_equal(u64(got["qber"]), u64(want_q)), "q differs from the reference's bits"
        assert np.array_equal(u64(got["log_p"]), u64([R.log_p(x) for x in want_q])), "log_p differs"
    return want_w


_dense_by_id = {}


def dense_of(H):
    if id(H) not in _dense_by_id:
        _dense_by_id[id(H)] = R.dense(H)
    return _dense_by_id[id(H)]


def noisy(H, batch, q, seed):
    a, b, _ = Q.bsc_frames(H.n, q, batch, seed=seed)
    return a, b, H.syndrome(a)


# ---- 1. weights (and q, log_p) equal the reference ---------------------------------
@pytest.mark.parametrize("name,batch", [("kat_n6_m4.dense", 3), ("s1_n10_m5.sp1", 1)])
def test_small_graphs(gpu_available, name, batch):
    H = load_fixture(name)
    rng = np.random.Generator(np.random.PCG64(5))
    alice = rng.integers(0, 2, (batch, H.n), dtype=np.uint8)
    bob = alice ^ (rng.random((batch, H.n)) < 0.2).astype(np.uint8)
    w = check_against_reference(Q.Graph(H), H, bob, H.syndrome(alice))
    assert w.shape == (batch,)


def test_c1_plain_and_blind_plan(gpu_available):
    H = load_fixture(C1)
    _, gb = c1_graphs()
    alice, bob, _, _, syn = c1_frames()
    w = check_against_reference(gb, H, bob, syn)
    assert np.unique(w).size > 5, "70 frames at QBER 0.02 spread over many weights"
    a, b, fill, _, _, syn_ext, _ = fixture()
    plan = gb.rate_plan(PUNCT, SHORT)
    assert np.array_equal(PUNCT, BLIND_PUNCT) and np.array_equal(SHORT, BLIND_SHORT)
    w = check_against_reference(gb, H, b, syn_ext, PUNCT, SHORT, plan)
    # rows of n_key entries hold the same keys: only the first n_key entries of a row are read
    junk = b.copy()
    junk[:, plan.n_key:] = 1
    assert np.array_equal(device_estimate(gb, junk, syn_ext, plan, want=("weight",))["weight"], w)


def test_shortened_only_plan_with_a_dead_row(gpu_available):
    H = load_fixture("u_n10_m5.dense")
    g = Q.Graph(H)
    short = u_plans()[0]
    plan = g.rate_plan([], short)
    rng = np.random.Generator(np.random.PCG64(9))
    bob = rng.integers(0, 2, (5, H.n), dtype=np.uint8)
    syn = rng.integers(0, 2, (5, H.m), dtype=np.uint8)  # (any syndrome: row 0 must not count whatever it holds)
    check_against_reference(g, H, bob, syn, None, short, plan)
    syn2 = syn.copy()
    syn2[:, 0] ^= 1
    assert np.array_equal(device_estimate(g, bob, syn2, plan, want=("weight",))["weight"],
                          device_estimate(g, bob, syn, plan, want=("weight",))["weight"])


def test_unaligned_keys_and_high_bits(gpu_available):
    import torch

    H = load_fixture(C1)
    _, gb = c1_graphs()
    _, bob, _, _, syn = c1_frames()
    want = R.weights(dense_of(H), bob, syn)
    # a view one byte into a larger buffer: pack_key_bits takes its byte path
    flat = torch.zeros(bob.size + 16, dtype=torch.uint8, device="cuda")
    flat[1:1 + bob.size] = cuda(bob).reshape(-1)
    view = flat[1:1 + bob.size].view(bob.shape)
    assert view.data_ptr() % 16 == 1
    got = device_estimate(gb, None, syn, d_keys=view, want=("weight",))
    assert np.array_equal(got["weight"], want)
    # 0xFE / 0xFF for 0 / 1: only bit 0 of key and syndrome bytes is read
    got = device_estimate(gb, bob | 0xFE, syn | 0xFE, want=("weight",))
    assert np.array_equal(got["weight"], want)
    assert np.array_equal(R.weights(dense_of(H), bob | 0xFE, syn | 0xFE), want)


@pytest.mark.parametrize("with_plan", [False, True])
def test_c2(gpu_available, with_plan):
    H = load_fixture(C2)
    g = Q.Graph(H)
    alice, bob, syn = noisy(H, 8, 0.0215, 3)
    if not with_plan:
        w = check_against_reference(g, H, bob, syn)
        q = device_estimate(g, bob, syn)["qber"]
        assert np.all(np.abs(q - 0.0215) < 0.006), "the estimate is nowhere near the channel"  # (5 sigma is 0.0056)
        return
    punct, short = c2_plan_lists()
    plan = g.rate_plan(punct, short)
    # Alice's syndrome of her extended key, with a private fill Bob never sees
    fill = np.random.Generator(np.random.PCG64(4)).integers(0, 2, (8, punct.size)).astype(np.uint8)
    _, syn_ext = g.syndrome(alice, plan, fill)
    check_against_reference(g, H, bob, syn_ext, punct, short, plan)


def test_split_layout_graph(gpu_available):
    H = load_fixture(C4S)
    g = Q.Graph(H)
    assert g.split_plan()["parts"] > 1
    alice, bob, syn = noisy(H, 2, 0.02, 8)
    w = check_against_reference(g, H, bob, syn, solve=False, csr=True)
    d = R.row_degrees_csr(H)
    deg, rows = np.unique(d[d > 0], return_counts=True)
    assert all(np.array_equal(x, y) for x, y in zip(g.estimate_classes(), (deg, rows)))
    got = device_estimate(g, bob, syn)
    want_q = [R.qber(deg, rows, k, Q_MIN, Q_MAX) for k in w]
    assert np.array_equal(u64(got["qber"]), u64(want_q))


def test_frame_per_lane_graph(gpu_available):
    H = load_fixture(C1)
    g = Q.Graph(H, layout="frame_per_lane")
    assert g.plan(0, Q.SPA)["variant"] == "fpl"
    _, bob, _, _, syn = c1_frames()
    check_against_reference(g, H, bob, syn)


def test_empty_batch(gpu_available):
    import torch

    H = load_fixture(C1)
    _, gb = c1_graphs()
    e = lambda *shape, dt=torch.uint8: torch.empty(shape, dtype=dt, device="cuda")  # noqa: E731
    gb.estimate_qber_device(e(0, H.n), e(0, H.m), e(0, dt=torch.int32), e(0, dt=torch.float64), e(0, dt=torch.float64))
    gb.corrected_errors_device(e(0, H.n), e(0, H.n), e(0, dt=torch.int32))
    q, lp, w = gb.estimate_qber(np.empty((0, H.n), np.uint8), np.empty((0, H.m), np.uint8))
    assert q.shape == lp.shape == w.shape == (0,)
    assert gb.corrected_errors(np.empty((0, H.n), np.uint8), np.empty((0, H.n), np.uint8)).shape == (0,)


# ---- 2. outputs ---------------------------------------------------------------------
@pytest.mark.parametrize("want", [("weight",), ("qber",), ("log_p",), ("weight", "log_p"), ("qber", "log_p"),
                                  ("weight", "qber")])
def test_each_output_may_be_missing(gpu_available, want):
    H = load_fixture(C1)
    _, gb = c1_graphs()
    _, bob, _, _, syn = c1_frames()
    full = device_estimate(gb, bob, syn)
    got = device_estimate(gb, bob, syn, want=want)
    assert set(got) == set(want)
    for k in want:
        assert np.array_equal(got[k].view(np.uint8), full[k].view(np.uint8)), k
    if want == ("weight",):  # nothing is solved: the bounds are not looked at
        assert np.array_equal(device_estimate(gb, bob, syn, want=want, q_min=0.0, q_max=0.9)["weight"], full["weight"])
    else:
        with pytest.raises(Q.QLDPCError, match="EINVAL.*q_min"):
            device_estimate(gb, bob, syn, want=want, q_min=0.0, q_max=0.9)


def test_all_outputs_missing_is_refused(gpu_available):
    _, gb = c1_graphs()
    _, bob, _, _, syn = c1_frames()
    with pytest.raises(Q.QLDPCError, match="EINVAL.*NULL device buffer"):
        gb.estimate_qber_device(cuda(bob), cuda(syn))


# ---- 3. the estimate feeds the decode on one stream ----------------------------------
@functools.lru_cache(maxsize=None)
def fed_decode():
    """C1, 16 frames, SPA capped at 20: estimate then reconcile on one side
    stream with nothing between them.  -> (bob, DecodeOutput, reference log_p)."""
    import torch

    H = load_fixture(C1)
    _, gb = c1_graphs()
    _, bob, _, _, syn = c1_frames()
    bob, syn = bob[:16], syn[:16]
    par = Q.Params(Q.SPA, 20, True, 100.0)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        d_bob, d_syn = cuda(bob), cuda(syn)
        lp = torch.full((16,), -7.5, dtype=torch.float64, device="cuda")
        bits = torch.empty((16, H.n), dtype=torch.uint8, device="cuda")
        it = torch.empty(16, dtype=torch.int32, device="cuda")
        ok = torch.empty(16, dtype=torch.uint8, device="cuda")
        post = torch.empty((16, H.n), dtype=torch.float64, device="cuda")
        gb.estimate_qber_device(d_bob, d_syn, None, None, lp, stream=side)
        gb.reconcile_device(par, d_bob, lp, d_syn, bits, it, ok, posterior=post, stream=side)
    side.synchronize()
    out = Q.DecodeOutput(bits.cpu().numpy(), it.cpu().numpy().astype(np.uint32), ok.cpu().numpy(), post.cpu().numpy())
    _, want_lp, _ = R.estimate(dense_of(H), bob, syn)
    assert np.array_equal(u64(lp.cpu().numpy()), u64(want_lp))
    return bob, out, want_lp, syn


def test_estimate_feeds_the_decode(gpu_available):
    H = load_fixture(C1)
    bob, out, want_lp, syn = fed_decode()
    O = Oracle(H)
    want = O.decode_batch(O.params(Q.SPA, 20, True, 100.0), np_llr(bob, want_lp), syn, threads=8, posterior=True)
    assert int(want[2].sum()) >= 3, "some frames must decode"
    assert_same(out, want, "reconcile fed by the estimate")


# ---- 4. corrected errors ---------------------------------------------------------------
def device_errors(g, keys, bits, plan=None):
    import torch

    batch = keys.shape[0]
    err = torch.full((batch + PAD,), -77, dtype=torch.int32, device="cuda")
    g.corrected_errors_device(cuda(keys), cuda(bits), err, plan=plan)
    torch.cuda.synchronize()
    h = err.cpu().numpy()
    assert np.all(h[batch:] == -77), "written past the batch"
    return h[:batch]


def test_corrected_errors_of_the_decoded_frames(gpu_available):
    _, gb = c1_graphs()
    bob, out, _, _ = fed_decode()
    got = device_errors(gb, bob, out.bits)
    assert got.dtype == np.int32 and np.array_equal(got, R.corrected_errors(bob, out.bits))
    alice = c1_frames()[0][:16]
    done = (out.bits == alice).all(axis=1)
    assert int(done.sum()) >= 3, "some frames must decode to Alice's key"
    assert np.array_equal(got[done], (alice ^ bob)[done].sum(axis=1)), "a corrected frame's count is its error count"
    assert np.array_equal(device_errors(gb, bob, bob), np.zeros(16, np.int32))
    assert np.array_equal(device_errors(gb, bob, bob ^ 1), np.full(16, gb.n, np.int32))
    assert np.array_equal(device_errors(gb, bob | 0xFE, out.bits | 0xFE), got), "only bit 0 is read"


def test_corrected_errors_odd_sizes(gpu_available):
    """Rows that are not 16-byte aligned, a length below one load, and a tail."""
    rng = np.random.Generator(np.random.PCG64(12))
    for name in ("kat_n6_m4.dense", "u_n10_m5.dense"):
        H = load_fixture(name)
        g = Q.Graph(H)
        k, b = rng.integers(0, 2, (5, H.n), dtype=np.uint8), rng.integers(0, 2, (5, H.n), dtype=np.uint8)
        assert np.array_equal(device_errors(g, k, b), R.corrected_errors(k, b))
        short = u_plans()[0] if name.startswith("u_") else np.array([2], np.int32)
        plan = g.rate_plan([0], short[short != 0])
        assert np.array_equal(device_errors(g, k, b, plan), R.corrected_errors(k, b, [0], short[short != 0]))


@functools.lru_cache(maxsize=None)
def blind_round0():
    """The blind fixture's round 0 (no disclosure): Bob's decode under the plan."""
    _, gb = c1_graphs()
    alg, prim, sec = ROUND_ALGS[0]
    _, bob, _, lp, _, syn, _ = fixture()
    plan = gb.rate_plan(PUNCT, SHORT)
    return gb.reconcile(Q.Params(alg, CAP, True, 100.0, prim, sec), bob, lp, syn, plan=plan), plan


def test_corrected_errors_under_a_plan(gpu_available):
    _, gb = c1_graphs()
    _, bob, _, _, ext, _, _ = fixture()
    out, plan = blind_round0()
    got = device_errors(gb, bob, out.bits, plan)
    assert np.array_equal(got, R.corrected_errors(bob, out.bits, PUNCT, SHORT))
    # punctured and shortened positions differ from Bob's row and must not count
    assert np.any(got != ((bob ^ out.bits) & 1).sum(axis=1))
    bob_ext = R.extend(bob, gb.n, PUNCT, SHORT)
    assert np.array_equal(device_errors(gb, bob, bob_ext, plan), np.zeros(bob.shape[0], np.int32))
    assert np.array_equal(device_errors(gb, bob, bob_ext ^ 1, plan), np.full(bob.shape[0], plan.n_key, np.int32))
    assert np.array_equal(device_errors(gb, bob, ext, plan), (bob[:, :plan.n_key] ^ ext[:, np.setdiff1d(
        np.arange(gb.n), np.concatenate([PUNCT, SHORT]))]).sum(axis=1)), "against Alice's extended key: the channel's errors"


# ---- 5. host entries, one shard and two ----------------------------------------------
@pytest.mark.parametrize("with_plan", [False, True])
def test_host_entries(gpu_available, with_plan):
    H = load_fixture(C1)
    _, gb = c1_graphs()
    g2 = Q.Graph(H, devices=[0, 0])
    if with_plan:
        _, bob, _, _, _, syn, _ = fixture()
        planb, plan2 = gb.rate_plan(PUNCT, SHORT), g2.rate_plan(PUNCT, SHORT)
        bits = blind_round0()[0].bits
    else:
        _, bob, _, _, syn = c1_frames()
        planb = plan2 = None
        bits = np.roll(bob, 1, axis=1)
    for batch in (5, 1):  # uneven shards, an empty shard
        dev = device_estimate(gb, bob[:batch], syn[:batch], planb)
        for g, plan in ((gb, planb), (g2, plan2)):
            q, lp, w = g.estimate_qber(bob[:batch], syn[:batch], plan)
            assert w.dtype == np.int32 and np.array_equal(w, dev["weight"])
            assert np.array_equal(u64(q), u64(dev["qber"])) and np.array_equal(u64(lp), u64(dev["log_p"]))
            e = g.corrected_errors(bob[:batch], bits[:batch], plan)
            assert e.dtype == np.int32 and np.array_equal(e, device_errors(gb, bob[:batch], bits[:batch], planb))
    # host entries with some outputs missing
    L = Q.lib()
    k, s = np.ascontiguousarray(bob[:5]), np.ascontiguousarray(syn[:5])
    w = np.full(5, -77, np.int32)
    ph = None if plan2 is None else plan2.handle
    assert L.qldpc_estimate_qber_batch(g2.handle, ph, 5, k.ctypes.data, s.ctypes.data, 0.0, 0.9, w.ctypes.data, None,
                                       None) == 0
    assert np.array_equal(w, device_estimate(gb, bob[:5], syn[:5], planb)["weight"])


# ---- 6. estimate.py ---------------------------------------------------------------------
def test_prior_per_frame_and_pooled(gpu_available):
    H = load_fixture(C1)
    _, gb = c1_graphs()
    _, bob, _, _, syn = c1_frames()
    D = dense_of(H)
    want_q, want_lp, want_w = R.estimate(D, bob, syn)
    q, lp, w = estimate.prior(gb, bob, syn)
    assert np.array_equal(w, want_w) and np.array_equal(u64(q), u64(want_q)) and np.array_equal(u64(lp), u64(want_lp))
    deg, cnt = R.classes(D)
    pooled = R.qber(deg, cnt, int(want_w.sum()), Q_MIN, Q_MAX, frames=bob.shape[0])
    q, lp, w = estimate.prior(gb, bob, syn, pooled=True)
    assert np.array_equal(w, want_w) and q.shape == (bob.shape[0],)
    assert np.all(u64(q) == u64(pooled)) and np.all(u64(lp) == u64(R.log_p(pooled)))
    assert abs(pooled - 0.02) < 0.002, "70 frames pooled: the estimate sits on the channel's QBER"


def test_block_qber_feeds_the_secret_length(gpu_available):
    """test_gpu_privacy's fixture: the blind fixture after one disclosure round.
    The verified frames' corrected errors give the block's QBER; both sides
    reach the same secret length from it."""
    import torch

    ga, gb = c1_graphs()
    alg, prim, sec = ROUND_ALGS[0]
    alice, bob, fill, lp, _, _, _ = fixture()
    plan_a, plan_b = ga.rate_plan(PUNCT, SHORT), gb.rate_plan(PUNCT, SHORT)
    res = Q.blind_reconcile(ga, plan_a, gb, plan_b, Q.Params(alg, CAP, True, 100.0, prim, sec), alice, bob, lp, fill,
                            STEP, max_rounds=1, q=QBER)
    n_key = plan_b.n_key
    d_key = torch.empty((alice.shape[0], n_key), dtype=torch.uint8, device="cuda")
    gb.extract_key_device(plan_b, cuda(res.bits), d_key)
    torch.cuda.synchronize()
    key_a, key_b = np.ascontiguousarray(alice[:, :n_key]), d_key.cpu().numpy()
    frames = np.flatnonzero((key_a == key_b).all(axis=1))
    assert 2 <= frames.size < alice.shape[0]
    errors = estimate.corrected_errors(gb, bob, res.bits, plan_b)
    q_b = estimate.block_qber(errors, n_key, frames)
    # Alice's count of the same frames: the channel's flips among her key bits
    flips = int((key_a[frames] ^ bob[frames, :n_key]).sum())
    assert q_b == flips / (frames.size * n_key) and 0.0 < q_b < 0.03
    leaked = privacy.leaked_bits(1024, 220, PUNCT.size, SHORT.size, res.disclosed)
    len_b = privacy.block_secret_length(n_key, leaked, frames, q_b, 64, 30)
    len_a = privacy.block_secret_length(n_key, leaked, frames, flips / (frames.size * n_key), 64, 30)
    assert len_a == len_b > 0
