"""The Toeplitz hash without a GPU: numpy's checker against an explicitly
built matrix, the argument checks of the two C entries through the LDS fit
(no device is touched before it), and the length bookkeeping of privacy.py on
hand-computed values."""
import numpy as np
import pytest

import qkd_ldpc_v_amd as Q
from qkd_ldpc_v_amd import QLDPCError, privacy
from toeplitz_ref import cut, toeplitz_ref

EINVAL, EUNSUP = -1, -5


def rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


# ---- numpy's checker ---------------------------------------------------------------------
@pytest.mark.parametrize("L,r", [(1, 1), (1, 4), (3, 5), (5, 3), (8, 8), (33, 7)])
def test_helper_is_the_toeplitz_matrix(L, r):
    g = rng(100 * L + r)
    keys = g.integers(0, 2, (3, L)).astype(np.uint8)
    seed = g.integers(0, 2, L + r - 1).astype(np.uint8)
    T = np.array([[seed[i - j + L - 1] for j in range(L)] for i in range(r)], np.int64)
    want = (keys.astype(np.int64) @ T.T) % 2
    assert np.array_equal(toeplitz_ref(keys, seed, r), want)


def test_helper_reads_bit_0_and_the_first_key_len_bytes():
    g = rng(5)
    keys = g.integers(0, 256, (4, 40)).astype(np.uint8)
    seed = g.integers(0, 256, 33 + 20 - 1 + 9).astype(np.uint8)  # (longer than needed: the tail is not read)
    want = toeplitz_ref(keys[:, :33] & 1, seed[:52] & 1, 20)
    assert np.array_equal(toeplitz_ref(keys, seed, 20, key_len=33), want)
    assert want.any() and not want.all()


def test_helper_prefix_property():
    g = rng(6)
    L, r = 37, 90
    keys = g.integers(0, 2, (5, L)).astype(np.uint8)
    seed = g.integers(0, 2, L + r - 1).astype(np.uint8)
    full = toeplitz_ref(keys, seed, r)
    for rp in (1, 31, 32, 33, 89):
        assert np.array_equal(toeplitz_ref(keys, seed[:L + rp - 1], rp), full[:, :rp])
    assert np.array_equal(cut(full, [0, 1, 32, 90, 89])[2], np.concatenate([full[2, :32], np.zeros(58, np.uint8)]))


# ---- the C entries' argument checks, in the header's order -----------------------------
def entries():
    """(name, call(batch, key_len, key_stride, keys, out_len, seed, out_lens, out)) of the two entries."""
    L = Q.lib()
    return [("device", lambda b, kl, ks, k, r, s, ol, o: L.qldpc_toeplitz_hash_device(b, kl, ks, k, r, s, ol, o, None)),
            ("host", lambda b, kl, ks, k, r, s, ol, o: L.qldpc_toeplitz_hash_batch(b, kl, ks, k, r, s, ol, o))]


def test_argument_checks_in_order():
    buf = np.zeros(64, np.uint8)  # a non-NULL pointer; none of these paths reads it
    p = buf.ctypes.data
    for name, call in entries():
        # counts first, whatever the pointers are — and before batch == 0
        for b in (0, 1, 5):
            assert call(-1, 8, 8, None, 4, None, None, None) == EINVAL, name
            assert call(b, 0, 8, None, 4, None, None, None) == EINVAL, name
            assert call(b, -3, 8, p, 4, p, None, p) == EINVAL, name
            assert call(b, 8, 8, None, 0, None, None, None) == EINVAL, name
            assert call(b, 8, 7, p, 4, p, None, p) == EINVAL, name
            assert "key_stride" in Q.lib().qldpc_last_error().decode()
        # an empty batch is done, NULL buffers and an oversized key included
        assert call(0, 8, 8, None, 4, None, None, None) == 0, name
        assert call(0, 8, 1 << 40, None, 4, None, None, None) == 0, name
        assert call(0, 2_000_000, 2_000_000, None, 4, None, None, None) == 0, name
        # NULL buffers before the LDS fit
        for k, s, o in ((None, p, p), (p, None, p), (p, p, None)):
            assert call(1, 8, 8, k, 4, s, None, o) == EINVAL, name
            assert call(1, 2_000_000, 2_000_000, k, 4, s, None, o) == EINVAL, name
        # the LDS fit: four frames' keys and the seed window as bit words in 160 KiB
        assert call(1, 2_000_000, 2_000_000, p, 4, p, None, p) == EUNSUP, name
        assert "LDS" in Q.lib().qldpc_last_error().decode()
        assert call(3, 261_889, 300_000, p, 1, p, None, p) == EUNSUP, name
        # (the device entry does not read d_out_len on the host: a pointer it could not read is no error here)
        assert call(1, 2_000_000, 2_000_000, p, 4, p, p, p) == EUNSUP, name


def test_host_entry_refuses_lengths_outside_the_row():
    g = rng(7)
    keys = g.integers(0, 2, (3, 40)).astype(np.uint8)
    seed = g.integers(0, 2, 40 + 16 - 1).astype(np.uint8)
    for bad in ([0, -1, 16], [17, 0, 0], [16, 16, 1 << 20]):
        with pytest.raises(QLDPCError, match="EINVAL.*out_lens") as e:
            Q.toeplitz_hash(keys, seed, 16, out_lens=bad)
        assert e.value.code == EINVAL
    with pytest.raises(QLDPCError, match="EINVAL.*out_lens"):  # (in range for 16 outputs, not for 8)
        Q.toeplitz_hash(keys, seed, 8, out_lens=[9, 0, 0])


def test_python_checks_shapes_before_the_call():
    keys, seed = np.zeros((2, 10), np.uint8), np.zeros(13, np.uint8)
    with pytest.raises(ValueError, match="seed holds 13"):
        Q.toeplitz_hash(keys, seed, 5)  # 10 + 5 - 1 = 14 entries are read
    with pytest.raises(ValueError, match="key_len"):
        Q.toeplitz_hash(keys, seed, 4, key_len=11)
    with pytest.raises(ValueError, match="out_lens"):
        Q.toeplitz_hash(keys, seed, 4, out_lens=[1, 2, 3])
    with pytest.raises(ValueError, match="lengths"):
        privacy.amplify(keys, seed, [1, -1])
    out, lens = privacy.amplify(keys, seed, [0, 0])  # nothing to hash: no call
    assert out.shape == (2, 0) and lens.dtype == np.int32
    assert Q.toeplitz_hash(np.zeros((0, 10), np.uint8), seed, 4).shape == (0, 4)  # batch == 0: no device either


# ---- lengths -------------------------------------------------------------------------------
def test_leaked_bits_is_the_efficiency_numerator():
    # C1 under the blind fixture's plan: 220 syndrome bits, 60 of them spent on punctured positions
    assert privacy.leaked_bits(1024, 220, 60, 4, [0, 20, 60]).tolist() == [160, 180, 220]
    assert int(privacy.leaked_bits(10, 5, 0, 0, 0)) == 5
    assert privacy.leaked_bits is Q.blind.leaked_bits
    d = np.array([0, 20, 40, 60])
    eff = Q.blind_efficiency(1024, 220, 60, 4, d, 0.016)
    assert np.array_equal(eff, (220 - 60 + d.astype(np.float64)) / (960 * Q.blind.h2(0.016)))


def test_secret_length_by_hand():
    # h2(1/4) = 1/2 + (3/4) log2(4/3) = 0.8112781244...: 1000 bits keep 188.72...
    assert abs(Q.blind.h2(0.25) - 0.8112781244591328) < 1e-15
    got = privacy.secret_length(1000, [0, 100, 104, 105, 5000], 0.25, 64, 20)
    assert got.dtype == np.int32 and got.tolist() == [104, 4, 0, 0, 0]  # 104.72, 4.72, 0.72, -0.28 and far below 0
    # q = 0 loses nothing to the phase-error term; q = 1/2 loses everything
    assert privacy.secret_length(1000, [0, 16], 0.0, 64, 20).tolist() == [916, 900]
    assert privacy.secret_length(1000, [0], 0.5, 0, 0).tolist() == [0]
    assert privacy.secret_length(1000, 0, 0.5, 0, 0).shape == ()
    # the blind fixture's figures: 960 (1 - h2(0.016)) = 846.38...; less 160 or 180 leaked, a 64-bit tag, 30 bits
    assert abs(960 * (1 - Q.blind.h2(0.016)) - 846.384) < 1e-3
    assert privacy.secret_length(960, [160, 180], 0.016, 64, 30).tolist() == [592, 572]


def test_verified_compares_rows():
    a = np.array([[0, 1, 1], [1, 1, 1], [0, 0, 0]], np.uint8)
    b = np.array([[0, 1, 1], [1, 0, 1], [0, 0, 0]], np.uint8)
    v = privacy.verified(a, b)
    assert v.dtype == np.uint8 and v.tolist() == [1, 0, 1]
    with pytest.raises(ValueError):
        privacy.verified(a, b[:, :2])
