"""The batched Toeplitz hash on the GPU (qldpc_toeplitz_hash_device / _batch,
privacy.py): every case bit for bit against numpy's checker (toeplitz_ref.py),
on random keys and seeds from fixed PCG64 seeds.

Shapes sit at the word edges of the kernel's bit words (a window offset of 0,
partly filled last words, more outputs than key bits), at its tile of 1024
outputs and its groups of four frames; the end-to-end case is the blind
fixture of test_gpu_blind.py stopped after one disclosure round."""
import functools

import numpy as np
import pytest

import qkd_ldpc_v_amd as Q
from qkd_ldpc_v_amd import privacy
from test_gpu_blind import BATCH, CAP, PUNCT, QBER, ROUND_ALGS, SHORT, STEP, fixture
from test_gpu_parties import c1_graphs, cuda
from toeplitz_ref import cut, toeplitz_ref

pytestmark = pytest.mark.gpu

GUARD = 0xA5
SHAPES = [(1, 1, 1), (31, 1, 2), (32, 32, 3), (33, 65, 3), (63, 64, 1), (64, 63, 5), (65, 130, 70), (960, 64, 70),
          (1024, 700, 70), (1000, 1500, 3), (10240, 2048, 4)]


def rand_bytes(seed, *shape):
    return np.random.Generator(np.random.PCG64(seed)).integers(0, 256, shape).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def case(key_len, out_len, batch, row_len=None):
    """Keys and seed (bytes 0..255) of a shape, and numpy's hash of their bit 0: computed once, never written."""
    keys = rand_bytes(1000 + key_len, batch, row_len or key_len)
    seed = rand_bytes(2000 + out_len, key_len + out_len - 1)
    want = toeplitz_ref(keys[:, :key_len] & 1, seed & 1, out_len)
    for a in (keys, seed, want):
        a.setflags(write=False)
    return keys, seed, want


def device_hash(keys, seed, out_len, out_lens=None, key_len=None, stream=None):
    """The device entry into a buffer pre-filled with 0xA5, one guard row after
    the last: -> the [batch, out_len] rows; the guard row is asserted intact."""
    import torch

    batch = keys.shape[0]
    buf = torch.full((batch + 1, out_len), GUARD, dtype=torch.uint8, device="cuda")
    d_lens = None if out_lens is None else cuda(np.asarray(out_lens, np.int32))
    Q.toeplitz_hash_device(cuda(keys), cuda(seed), buf[:batch], d_lens, key_len=key_len, stream=stream)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert (got[batch] == GUARD).all(), "the row after the last was written"
    return got[:batch]


@pytest.mark.parametrize("key_len,out_len,batch", SHAPES)
def test_shapes_at_the_word_edges(gpu_available, key_len, out_len, batch):
    keys, seed, want = case(key_len, out_len, batch)
    if key_len * batch >= 64:  # (bytes above 1 among the keys, and a hash that is neither all 0 nor all 1)
        assert keys.max() > 1 and 0 < want.mean() < 1
    got = device_hash(keys, seed, out_len)
    assert got.max() <= 1, "outputs are 0 or 1"
    assert np.array_equal(got, want)


def test_longest_key_the_lds_holds(gpu_available):
    """key_len 261,888 fills the 160 KiB of LDS to the byte; one bit more is
    refused before the device is touched (tests/test_privacy_host.py)."""
    keys, seed, want = case(261_888, 3, 5)
    assert np.array_equal(device_hash(keys, seed, 3), want)


@pytest.mark.parametrize("row_len", [1024, 970])  # 16-byte aligned rows (wide loads) and rows that are not
def test_key_stride_longer_than_the_key(gpu_available, row_len):
    keys, seed, want = case(960, 64, 70, row_len)
    assert keys[:, 960:].any(), "the padding must not be zero"
    assert np.array_equal(device_hash(keys, seed, 64, key_len=960), want)
    assert np.array_equal(Q.toeplitz_hash(keys, seed, 64, key_len=960), want)
    assert np.array_equal(want, toeplitz_ref(np.ascontiguousarray(keys[:, :960]), seed, 64))


@pytest.mark.parametrize("key_len,out_len,batch,extra", [(1024, 700, 70, ()), (200, 2100, 9, (1023, 1024, 1025))])
def test_per_frame_lengths(gpu_available, key_len, out_len, batch, extra):
    """Row f is the full hash's first out_lens[f] bits, then zeros, in a buffer
    pre-filled with 0xA5; the second shape has lengths on both sides of the
    tile of 1024 outputs."""
    keys, seed, want = case(key_len, out_len, batch)
    values = np.array((0, 1, 63, 64, 65, out_len) + extra)
    lens = np.random.Generator(np.random.PCG64(77)).choice(values, batch)
    lens[:values.size] = values  # every value occurs
    got = device_hash(keys, seed, out_len, lens)
    assert np.array_equal(got, cut(want, lens))
    assert np.array_equal(Q.toeplitz_hash(keys, seed, out_len, out_lens=lens), cut(want, lens))
    # the device entry clamps: -1 is 0 and out_len + 5 is out_len
    odd = lens.copy()
    odd[[0, batch - 1]] = -1, out_len + 5
    clamped = np.clip(odd, 0, out_len)
    assert clamped[0] == 0 and clamped[-1] == out_len
    assert np.array_equal(device_hash(keys, seed, out_len, odd), cut(want, clamped))
    # a batch of zero lengths is all zero (no workgroup hashes anything)
    assert not device_hash(keys, seed, out_len, np.zeros(batch, np.int32)).any()


def test_prefix_property_on_the_device(gpu_available):
    keys, seed, want = case(1000, 1500, 3)
    for rp in (1, 64, 700, 1024, 1025):
        got = device_hash(keys, np.ascontiguousarray(seed[:1000 + rp - 1]), rp)
        assert np.array_equal(got, want[:, :rp]), rp


def test_streams_and_the_host_entry_agree(gpu_available):
    import torch

    keys, seed, want = case(1024, 700, 70)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):  # (the inputs are uploaded on the stream that reads them)
        on_side = device_hash(keys, seed, 700, stream=side)
    on_default = device_hash(keys, seed, 700)
    host = Q.toeplitz_hash(keys, seed, 700)
    assert np.array_equal(on_side, want) and np.array_equal(on_default, want) and np.array_equal(host, want)
    assert np.array_equal(privacy.tag(keys, seed, 64), want[:, :64])  # the tag is the hash's prefix


def test_verify_and_amplify_after_one_blind_round(gpu_available):
    """The blind fixture stopped after one disclosure round: a good part of the
    batch is still wrong.  The 64-bit tags tell exactly the frames whose keys
    are equal; those are amplified to the same bits on both sides, to lengths
    that differ by the 20 bits disclosed to the frames of round 1."""
    import torch

    ga, gb = c1_graphs()
    alg, prim, sec = ROUND_ALGS[0]
    alice, bob, fill, lp, _, _, _ = fixture()
    plan_a, plan_b = ga.rate_plan(PUNCT, SHORT), gb.rate_plan(PUNCT, SHORT)
    res = Q.blind_reconcile(ga, plan_a, gb, plan_b, Q.Params(alg, CAP, True, 100.0, prim, sec), alice, bob, lp, fill,
                            STEP, max_rounds=1, q=QBER)
    n_key = plan_b.n_key
    assert n_key == 960
    d_key = torch.full((BATCH, n_key), 7, dtype=torch.uint8, device="cuda")
    gb.extract_key_device(plan_b, cuda(res.bits), d_key)
    torch.cuda.synchronize()
    key_b = d_key.cpu().numpy()
    key_a = np.ascontiguousarray(alice[:, :n_key])  # (the first n_key entries of her rows are her key)
    equal = (key_a == key_b).all(axis=1)
    assert equal.sum() >= 2 and (~equal).sum() >= 2, "the fixture must leave both kinds of frames"

    tag_seed = rand_bytes(31, n_key + 64 - 1)
    tag_a, tag_b = privacy.tag(key_a, tag_seed), privacy.tag(key_b, tag_seed)
    assert tag_a.shape == (BATCH, 64)
    ok = privacy.verified(tag_a, tag_b)
    assert np.array_equal(ok, equal.astype(np.uint8)), "the tags must tell equal keys from unequal ones"
    # (syndromes_match is not that: a frame may fail its syndrome, or pass it on a wrong codeword)
    # the device entry on Alice's [batch][n] rows, of which the first n_key count, gives her tag
    assert np.array_equal(device_hash(alice, tag_seed, 64, key_len=n_key), tag_a)

    lengths = privacy.secret_length(n_key, privacy.leaked_bits(1024, 220, PUNCT.size, SHORT.size, res.disclosed),
                                    QBER, 64, 30)
    lengths[ok == 0] = 0
    assert np.unique(lengths[lengths > 0]).size >= 2, "round 0 and round 1 frames differ by the disclosed bits"
    assert set(np.unique(lengths[lengths > 0])) <= {592, 572}
    pa_seed = rand_bytes(32, n_key + int(lengths.max()) - 1)
    out_a, len_a = privacy.amplify(key_a, pa_seed, lengths)
    out_b, len_b = privacy.amplify(key_b, pa_seed, lengths)
    assert out_a.shape == (BATCH, int(lengths.max())) and np.array_equal(len_a, lengths) and np.array_equal(len_b, lengths)
    assert np.array_equal(out_a[ok == 1], out_b[ok == 1])
    assert np.array_equal(out_b, cut(toeplitz_ref(key_b, pa_seed, int(lengths.max())), lengths))
    assert not out_a[ok == 0].any() and not out_b[ok == 0].any()
