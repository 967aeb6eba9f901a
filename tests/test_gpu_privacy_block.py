"""The block hash on the GPU (qldpc_toeplitz_hash_block_device / _block,
privacy.block_*): every output bit for bit against numpy's block reference
(toeplitz_block_ref.py, a float64 FFT whose rounding is asserted), against the
existing checker toeplitz_ref where L * r <= 2 * 10^7, and against the index
formula itself (toeplitz_at) at the sizes beyond both.

The decomposition these shapes walk: a transform of N = 2^k points runs its
lowest min(k, 12) stages on one LDS tile per workgroup and the k - 12 stages
above in ceil((k - 12) / 7) strided passes.  k = 13 is the first size with a
strided pass (of one stage), k = 20 the first with two (4 + 4 stages), k = 27
the first with three (5 + 5 + 5); below k = 9 a tile is smaller than the
workgroup's 512 butterflies, at k = 0 it is one point and no stage runs.

Keys and seeds are random bytes from fixed PCG64 seeds: their upper bits show
that only bit 0 is read."""
import functools

import numpy as np
import pytest

import qkd_ldpc_v_amd as Q
from qkd_ldpc_v_amd import QLDPCError, privacy
from test_gpu_blind import BATCH, CAP, PUNCT, QBER, ROUND_ALGS, SHORT, STEP, fixture
from test_gpu_parties import c1_graphs, cuda
from toeplitz_block_ref import block_of, toeplitz_at, toeplitz_block_ref
from toeplitz_ref import toeplitz_ref

pytestmark = pytest.mark.gpu

GUARD = 0xA5
EINVAL = -1


def rand_bytes(seed, *shape):
    return np.random.Generator(np.random.PCG64(seed)).integers(0, 256, shape, dtype=np.uint8)


def device_block(keys, seed, out_len, frames=None, key_len=None, workspace=None, stream=None):
    """The device entry into a buffer pre-filled with 0xA5 with 64 guard bytes after out_len: -> the
    outputs; the guard is asserted intact."""
    import torch

    buf = torch.full((out_len + 64,), GUARD, dtype=torch.uint8, device="cuda")
    d_frames = None if frames is None else cuda(np.asarray(frames, np.int32))
    Q.toeplitz_hash_block_device(cuda(keys) if isinstance(keys, np.ndarray) else keys,
                                 cuda(seed) if isinstance(seed, np.ndarray) else seed, buf[:out_len], d_frames,
                                 key_len=key_len, workspace=workspace, stream=stream)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert (got[out_len:] == GUARD).all(), "bytes after out_len were written"
    assert got[:out_len].max() <= 1, "outputs are 0 or 1"
    return got[:out_len]


def check_block(keys, seed, out_len, frames=None, key_len=None, **kw):
    """device == numpy's block reference (and the existing checker where it is affordable) -> the outputs"""
    key_len = keys.shape[1] if key_len is None else key_len
    x = block_of(keys, frames, key_len)
    want = toeplitz_block_ref(x, seed, out_len)
    if x.size * out_len <= 2 * 10**7:
        assert np.array_equal(want, toeplitz_ref(x, seed, out_len)[0])
    got = device_block(keys, seed, out_len, frames, key_len, **kw)
    assert np.array_equal(got, want), f"L={x.size} r={out_len}: {np.flatnonzero(got != want)[:8]} differ"
    return got


# ---- 1. every transform size ------------------------------------------------------------------
def split(total, key_heavy):
    """(n_list, key_len, out_len) with n_list * key_len + out_len - 1 == total: about 3/4 of it key (or 1/4),
    the key an odd number of bits per frame."""
    key_len = 1 if total < 200 else 33 if total < 40000 else 1021
    n_list = max(1, (3 * total // 4 if key_heavy else total // 4) // key_len)
    return n_list, key_len, total - n_list * key_len + 1


@pytest.mark.parametrize("k", range(1, 23))
def test_every_transform_size(gpu_available, k):
    N = 1 << k
    for total in (N, N - 1, N // 2 + 1):  # exactly N; one short of it; the first length that needs this N
        for key_heavy in (True, False):
            n_list, key_len, out_len = split(total, key_heavy)
            assert n_list * key_len + out_len - 1 == total and out_len >= 1
            keys = rand_bytes(100 * k + key_heavy, n_list, key_len)
            seed = rand_bytes(100 * k + 50 + key_heavy, total)
            got = check_block(keys, seed, out_len)
            if total >= 256:
                assert 0.3 < got.mean() < 0.7


# ---- 2. extremes ---------------------------------------------------------------------------------
@pytest.mark.parametrize("L,r", [(1, 1), (1, 5000), (5000, 1)])
def test_degenerate_shapes(gpu_available, L, r):
    check_block(rand_bytes(L + 2, 1, L), rand_bytes(r, L + r - 1), r)


@pytest.mark.parametrize("L", [(1 << 22) - 1001, (1 << 22) - 1000])  # odd, even
def test_all_ones_is_the_largest_count(gpu_available, L):
    import torch

    r = 1001
    keys = torch.full((1, L), 0xFF, dtype=torch.uint8, device="cuda")
    seed = torch.full((L + r - 1,), 0xFF, dtype=torch.uint8, device="cuda")
    assert (device_block(keys, seed, r) == (L & 1)).all()  # every count is L


def test_the_limit_all_ones(gpu_available):
    import torch

    L, r = (1 << 27) - 1000, 1001  # N = 2^27: L + r - 1 is the limit itself; 8 frames of 2^24 - 125 bits
    keys = torch.ones((8, L // 8), dtype=torch.uint8, device="cuda")
    seed = torch.ones((L + r - 1,), dtype=torch.uint8, device="cuda")
    assert (device_block(keys, seed, r) == (L & 1)).all()
    with pytest.raises(QLDPCError, match="EUNSUP"):
        Q.toeplitz_block_workspace(L, r + 1)


def test_the_limit_random(gpu_available):
    L, r = (1 << 27) - 1000, 1001
    x, s = rand_bytes(271, 8, L // 8), rand_bytes(272, L + r - 1)
    got = device_block(x, s, r)
    idx = np.array([0, 1, 63, 64, 500, 777, r - 2, r - 1])
    assert np.array_equal(got[idx], toeplitz_at(block_of(x, None, L // 8), s, idx))
    assert 0.4 < got.mean() < 0.6


# ---- 3. the gather ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def gather_case():
    keys, seed = rand_bytes(31, 40, 1100), rand_bytes(32, 40 * 1021 + 3000 - 1)
    for a in (keys, seed):
        a.setflags(write=False)
    return keys, seed


@pytest.mark.parametrize("frames", [None, list(range(39, -1, -1)), [7, 3, 3, 30, 0, 7, 7], [5],
                                    list(np.random.Generator(np.random.PCG64(9)).permutation(40)[:17])])
def test_gather_follows_the_list(gpu_available, frames):
    """Permuted lists, repeated frames, no list at all; rows of 1100 bytes of which 1021 are key, the pad
    bytes random."""
    keys, seed = gather_case()
    assert keys[:, 1021:].any() and keys.max() > 1 and seed.max() > 1
    got = check_block(keys, seed, 3000, frames, key_len=1021)
    if frames is not None and list(frames) != sorted(frames):  # the order counts: the sorted list hashes otherwise
        assert not np.array_equal(got, device_block(keys, seed, 3000, sorted(frames), key_len=1021))
    assert np.array_equal(Q.toeplitz_hash_block(keys, seed, 3000, frames=frames, key_len=1021), got)


# ---- 4. agreement with what exists ------------------------------------------------------------
def test_one_frame_block_is_the_per_frame_hash(gpu_available):
    import torch

    keys, seed = gather_case()
    per_frame = torch.empty((40, 700), dtype=torch.uint8, device="cuda")
    Q.toeplitz_hash_device(cuda(keys), cuda(seed), per_frame, key_len=1021)
    per_frame = per_frame.cpu().numpy()
    for f in (0, 17, 39):
        assert np.array_equal(device_block(keys, seed, 700, [f], key_len=1021), per_frame[f])


def test_prefix_property(gpu_available):
    keys, seed = gather_case()
    frames, L = [4, 2, 9], 3 * 1021
    full = check_block(keys, seed, 3000, frames, key_len=1021)
    for rp in (1, 64, 1034, 2999):  # (1034: L + rp - 1 = 4096, a smaller transform than the full hash's)
        got = device_block(keys, np.ascontiguousarray(seed[:L + rp - 1]), rp, frames, key_len=1021)
        assert np.array_equal(got, full[:rp]), rp


# ---- 5. the workspace and the bounds ----------------------------------------------------------
def test_workspace_is_scratch_and_bounds_hold(gpu_available):
    import torch

    keys, seed = gather_case()
    shape_a = dict(frames=[1, 2, 3, 4, 5], out_len=3000)   # N = 8192
    shape_b = dict(frames=list(range(40)), out_len=1500)   # N = 65536: every byte shape_a used is overwritten
    need = {n: Q.toeplitz_block_workspace(len(s["frames"]) * 1021, s["out_len"]) for n, s in
            (("a", shape_a), ("b", shape_b))}
    assert need["a"] < need["b"]
    buf = torch.full((need["b"] + 256,), 0xFF, dtype=torch.uint8, device="cuda")

    def run(shape, n):
        got = check_block(keys, seed, shape["out_len"], shape["frames"], key_len=1021, workspace=buf[:need[n]])
        assert (buf[need[n]:].cpu().numpy() == 0xFF).all(), "bytes after ws_bytes were written"
        return got

    first = run(shape_a, "a")     # on a workspace of 0xFF
    run(shape_b, "b")             # another shape on the same bytes
    buf[need["a"]:] = 0xFF
    assert np.array_equal(run(shape_a, "a"), first)  # on what shape_b left behind
    # one byte short: refused, and the output is not touched
    out = torch.full((3000,), GUARD, dtype=torch.uint8, device="cuda")
    with pytest.raises(QLDPCError, match=f"EINVAL.*{need['a']}") as e:
        Q.toeplitz_hash_block_device(cuda(keys), cuda(seed), out, cuda(np.array(shape_a["frames"], np.int32)),
                                     key_len=1021, workspace=buf[:need["a"] - 1])
    assert e.value.code == EINVAL
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == GUARD).all()


# ---- 6. streams, the host entry, privacy.py ---------------------------------------------------
def test_streams_host_entry_and_privacy_agree(gpu_available):
    import torch

    keys, seed = gather_case()
    frames = [11, 0, 25, 3]
    want = toeplitz_block_ref(block_of(keys[:, :1021], frames, 1021), seed, 2000)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):  # (the inputs are uploaded on the stream that reads them)
        on_side = device_block(keys, seed, 2000, frames, key_len=1021, stream=side)
    on_default = device_block(keys, seed, 2000, frames, key_len=1021)
    host = Q.toeplitz_hash_block(keys, seed, 2000, frames=frames, key_len=1021)
    assert np.array_equal(on_side, want) and np.array_equal(on_default, want) and np.array_equal(host, want)
    cut = np.ascontiguousarray(keys[:, :1021])  # (privacy.py hashes whole rows)
    assert np.array_equal(privacy.block_tag(cut, seed, frames), want[:64])  # the tag is the hash's prefix
    assert np.array_equal(privacy.block_tag(cut, seed, frames, 100), want[:100])
    assert np.array_equal(privacy.block_amplify(cut, seed, frames, 2000), want)


# ---- 7. the protocol ----------------------------------------------------------------------------
def test_block_verify_and_amplify_after_one_blind_round(gpu_available):
    """The blind fixture stopped after one disclosure round.  The frames whose per-frame tags agree make
    one block: both sides amplify it to the same block_secret_length bits, numpy's too; with one
    unverified frame in the list the two sides' block tags differ."""
    import torch

    ga, gb = c1_graphs()
    alg, prim, sec = ROUND_ALGS[0]
    alice, bob, fill, lp, _, _, _ = fixture()
    plan_a, plan_b = ga.rate_plan(PUNCT, SHORT), gb.rate_plan(PUNCT, SHORT)
    res = Q.blind_reconcile(ga, plan_a, gb, plan_b, Q.Params(alg, CAP, True, 100.0, prim, sec), alice, bob, lp, fill,
                            STEP, max_rounds=1, q=QBER)
    n_key = plan_b.n_key
    d_key = torch.full((BATCH, n_key), 7, dtype=torch.uint8, device="cuda")
    gb.extract_key_device(plan_b, cuda(res.bits), d_key)
    torch.cuda.synchronize()
    key_b = d_key.cpu().numpy()
    key_a = np.ascontiguousarray(alice[:, :n_key])
    tag_seed = rand_bytes(31, n_key + 64 - 1)
    ok = privacy.verified(privacy.tag(key_a, tag_seed), privacy.tag(key_b, tag_seed))
    frames, bad = np.flatnonzero(ok == 1), np.flatnonzero(ok == 0)
    assert frames.size >= 2 and bad.size >= 1, "the fixture must leave both kinds of frames"

    leaked = privacy.leaked_bits(1024, 220, PUNCT.size, SHORT.size, res.disclosed)
    length = privacy.block_secret_length(n_key, leaked, frames, QBER, 64, 30)
    per_frame = privacy.secret_length(n_key, leaked, QBER, 64, 30)[frames]
    assert length == int(np.floor(frames.size * n_key * (1 - Q.blind.h2(QBER)) - leaked[frames].sum() - 94))
    assert length >= per_frame.sum() + 94 * (frames.size - 1)  # one tag and one margin, not n_list of them
    pa_seed = rand_bytes(33, frames.size * n_key + length - 1)
    out_a = privacy.block_amplify(key_a, pa_seed, frames, length)
    out_b = privacy.block_amplify(key_b, pa_seed, frames, length)
    assert out_a.shape == (length,) and np.array_equal(out_a, out_b)
    assert np.array_equal(out_b, toeplitz_block_ref(block_of(key_b, frames, n_key), pa_seed, length))

    block_seed = rand_bytes(34, (frames.size + 1) * n_key + 64 - 1)
    assert np.array_equal(privacy.block_tag(key_a, block_seed, frames), privacy.block_tag(key_b, block_seed, frames))
    with_bad = np.append(frames, bad[0])
    tag_a, tag_b = privacy.block_tag(key_a, block_seed, with_bad), privacy.block_tag(key_b, block_seed, with_bad)
    assert tag_a.shape == (64,) and not np.array_equal(tag_a, tag_b)


# ---- 8. the workload's shape --------------------------------------------------------------------
def test_the_c2_batch_as_one_block(gpu_available):
    """4096 frames of 10240 bits, out_len 2^24: N = 2^26, two strided passes of 7 stages."""
    batch, n_key, r = 4096, 10240, 1 << 24
    keys, seed = rand_bytes(81, batch, n_key), rand_bytes(82, batch * n_key + r - 1)
    got = device_block(keys, seed, r)
    idx = np.array([0, 1, 4095, 4096, 1 << 20, 12345678, r - 2, r - 1])
    assert np.array_equal(got[idx], toeplitz_at(keys.reshape(-1), seed, idx))
    assert 0.49 < got.mean() < 0.51
