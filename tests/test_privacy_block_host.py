"""The block hash without a GPU: numpy's block reference against the existing
checker and against the index formula itself, the argument checks of the two
C entries in the header's order (no device is touched through them), the
workspace size, the Python wrappers' checks and the block's length
bookkeeping on hand-computed values."""
import numpy as np
import pytest

import qkd_ldpc_v_amd as Q
from qkd_ldpc_v_amd import QLDPCError, privacy
from toeplitz_block_ref import block_of, toeplitz_at, toeplitz_block_ref
from toeplitz_ref import toeplitz_ref

EINVAL, EUNSUP = -1, -5
LIMIT = 1 << 27


def rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


# ---- numpy's block reference ---------------------------------------------------------------
@pytest.mark.parametrize("L,r", [(1, 1), (33, 20), (1000, 49), (4097, 4096), (70000, 300)])
def test_block_reference_is_the_existing_checker(L, r):
    g = rng(L + r)
    x = g.integers(0, 256, L).astype(np.uint8)  # (bytes above 1: only bit 0 counts)
    s = g.integers(0, 256, L + r - 1 + 3).astype(np.uint8)  # (longer than needed: the tail is not read)
    assert np.array_equal(toeplitz_block_ref(x, s, r), toeplitz_ref(x, s, r)[0])


def test_block_reference_is_the_formula_at_a_large_size():
    L, r = (1 << 22) - 1000, 1001
    g = rng(22)
    x, s = g.integers(0, 2, L).astype(np.uint8), g.integers(0, 2, L + r - 1).astype(np.uint8)
    idx = np.concatenate([[0, r - 1], g.choice(np.arange(1, r - 1), 30, replace=False)])
    want = toeplitz_at(x, s, idx)
    assert 0 < want.mean() < 1
    assert np.array_equal(toeplitz_block_ref(x, s, r)[idx], want)


def test_block_of_follows_the_list():
    keys = rng(3).integers(0, 256, (5, 7)).astype(np.uint8)
    assert np.array_equal(block_of(keys, None, 7), (keys & 1).reshape(-1))
    got = block_of(keys, [3, 0, 3], 4)
    assert np.array_equal(got, np.concatenate([keys[3, :4], keys[0, :4], keys[3, :4]]) & 1)


# ---- the C entries' argument checks, in the header's order ---------------------------------
def entries():
    """(name, call(n_list, key_len, key_stride, keys, out_len, seed, out, ws, ws_bytes)) of the two entries;
    the host entry's batch is n_list + 2 and its list NULL."""
    L = Q.lib()
    return [("device", lambda n, kl, ks, k, r, s, o, ws, wb: L.qldpc_toeplitz_hash_block_device(n, None, kl, ks, k, r, s,
                                                                                               o, ws, wb, None)),
            ("host", lambda n, kl, ks, k, r, s, o, ws, wb: L.qldpc_toeplitz_hash_block(n + 2, n, None, kl, ks, k, r, s,
                                                                                       o))]


def test_argument_checks_in_order():
    buf = np.zeros(64, np.uint8)  # a non-NULL pointer; none of these paths reads it
    p = buf.ctypes.data
    lib = Q.lib()
    for name, call in entries():
        # (1) counts first, whatever the pointers are — and before n_list == 0
        for n in (0, 1, 5):
            assert call(-1, 8, 8, None, 4, None, None, None, 0) == EINVAL, name
            assert call(n, 0, 8, None, 4, None, None, None, 0) == EINVAL, name
            assert call(n, -3, 8, p, 4, p, p, p, 64) == EINVAL, name
            assert call(n, 8, 8, None, 0, None, None, None, 0) == EINVAL, name
            assert call(n, 8, 8, p, -1, p, p, p, 64) == EINVAL, name
            assert call(n, 8, 7, p, 4, p, p, p, 64) == EINVAL, name
            assert "key_stride" in lib.qldpc_last_error().decode()
        # (2) an empty list is done: NULL buffers, an oversized block's shape and no workspace included
        assert call(0, 8, 8, None, 4, None, None, None, 0) == 0, name
        assert call(0, 8, 1 << 40, None, 1 << 40, None, None, None, 0) == 0, name
        # (3) NULL buffers before the size limit
        for k, s, o in ((None, p, p), (p, None, p), (p, p, None)):
            assert call(1, 8, 8, k, 4, s, o, p, 64) == EINVAL, name
            assert call(1 << 20, 1 << 20, 1 << 20, k, 4, s, o, p, 64) == EINVAL, name
        # (4) the limit: L + out_len - 1 <= 2^27
        assert call(1 << 20, 1 << 20, 1 << 20, p, 4, p, p, p, 64) == EUNSUP, name
        assert "2^27" in lib.qldpc_last_error().decode()
        assert call(1, LIMIT, LIMIT, p, 2, p, p, p, 64) == EUNSUP, name
        assert call(1 << 7, 1 << 20, 1 << 20, p, 2, p, p, p, 64) == EUNSUP, name
        assert call(1, 8, 8, p, 1 << 40, p, p, p, 64) == EUNSUP, name
    dev, host = (c for _, c in entries())
    # the host entry's own counts: batch < 0, n_list > batch — before n_list == 0 and the pointers
    assert lib.qldpc_toeplitz_hash_block(-1, 0, None, 8, 8, None, 4, None, None) == EINVAL
    assert lib.qldpc_toeplitz_hash_block(2, 3, None, 8, 8, None, 4, None, None) == EINVAL
    assert "batch" in lib.qldpc_last_error().decode()
    # (3) the device entry's workspace pointer, (5) its size — after the limit, with the size needed in the message
    assert dev(1, 8, 8, p, 4, p, p, None, 1 << 30) == EINVAL
    assert dev(1, LIMIT, LIMIT, p, 2, p, p, p, 0) == EUNSUP
    need = lib.qldpc_toeplitz_block_workspace(8, 4)
    assert dev(1, 8, 8, p, 4, p, p, p, need - 1) == EINVAL
    assert str(need) in lib.qldpc_last_error().decode()
    # (6) the host entry's list entries: after the limit, before any device
    bad = np.array([0, 3, 1], np.int32)
    assert lib.qldpc_toeplitz_hash_block(3, 3, bad.ctypes.data, LIMIT, LIMIT, p, 2, p, p) == EUNSUP
    assert lib.qldpc_toeplitz_hash_block(3, 3, bad.ctypes.data, 8, 8, p, 4, p, p) == EINVAL
    assert "list[1]" in lib.qldpc_last_error().decode()
    bad[1] = -1
    assert lib.qldpc_toeplitz_hash_block(3, 3, bad.ctypes.data, 8, 8, p, 4, p, p) == EINVAL


def test_workspace_size():
    lib = Q.lib()
    sizes = []
    for total in (1, 2, 3, 4, 5, 1000, 4096, 4097, 1 << 20, (1 << 20) + 1, 1 << 26, LIMIT - 1, LIMIT):
        for L in {1, (total + 1) // 2, total}:  # (any split of L + out_len - 1 = total asks for the same)
            sizes.append((total, lib.qldpc_toeplitz_block_workspace(L, total - L + 1)))
    assert all(b > 0 for _, b in sizes)
    for (t0, b0), (t1, b1) in zip(sizes, sizes[1:]):
        assert b1 >= b0 if t1 >= t0 else True, (t0, t1)
    assert sizes[0][1] < sizes[-1][1]
    assert Q.toeplitz_block_workspace(1000, 25) == lib.qldpc_toeplitz_block_workspace(1000, 25)
    # three arrays of N words hold everything: two transforms and the table
    assert Q.toeplitz_block_workspace(LIMIT - 1000, 1001) >= 3 * 4 * LIMIT
    assert lib.qldpc_toeplitz_block_workspace(LIMIT, 2) == EUNSUP
    assert lib.qldpc_toeplitz_block_workspace(1, LIMIT + 1) == EUNSUP
    assert lib.qldpc_toeplitz_block_workspace(1 << 40, 1 << 40) == EUNSUP
    assert lib.qldpc_toeplitz_block_workspace(0, 4) == EINVAL and lib.qldpc_toeplitz_block_workspace(4, 0) == EINVAL
    with pytest.raises(QLDPCError, match="EUNSUP"):
        Q.toeplitz_block_workspace(LIMIT, 2)


# ---- the Python wrappers ----------------------------------------------------------------------
def test_python_checks_shapes_before_the_call():
    keys, seed = np.zeros((3, 10), np.uint8), np.zeros(33, np.uint8)
    with pytest.raises(ValueError, match="seed holds 33"):
        Q.toeplitz_hash_block(keys, seed, 5)  # 3 * 10 + 5 - 1 = 34 entries are read
    with pytest.raises(ValueError, match="seed holds 33"):
        Q.toeplitz_hash_block(keys, seed, 25, frames=[0])  # 10 + 25 - 1
    with pytest.raises(ValueError, match="key_len"):
        Q.toeplitz_hash_block(keys, seed, 4, key_len=11)
    with pytest.raises(ValueError, match="out_len"):
        Q.toeplitz_hash_block(keys, seed, 0)
    for bad in ([0, 3], [-1], [1, 2, 1 << 20]):
        with pytest.raises(ValueError, match="frames"):
            Q.toeplitz_hash_block(keys, seed, 4, frames=bad)
    with pytest.raises(ValueError, match="frames"):
        Q.toeplitz_hash_block(keys, np.zeros(100, np.uint8), 4, frames=[0, 0, 1, 1])  # (more entries than rows)
    with pytest.raises(ValueError, match="length"):
        privacy.block_amplify(keys, seed, [0], -1)
    assert privacy.block_amplify(keys, seed, [0, 1], 0).shape == (0,)  # nothing to hash: no call


def test_device_wrapper_checks_before_the_call():
    """The device wrapper's checks need no device: host tensors never reach the C entry here."""
    import torch

    keys, seed, out = torch.zeros((3, 10), dtype=torch.uint8), torch.zeros(33, dtype=torch.uint8), torch.zeros(5, dtype=torch.uint8)
    with pytest.raises(ValueError, match="seed holds 33"):
        Q.toeplitz_hash_block_device(keys, seed, out)  # 3 * 10 + 5 - 1 = 34 entries are read
    with pytest.raises(ValueError, match="key_len"):
        Q.toeplitz_hash_block_device(keys, seed, out[:4], key_len=11)
    with pytest.raises(ValueError, match="int32"):
        Q.toeplitz_hash_block_device(keys, seed, out[:4], frames=torch.zeros(2, dtype=torch.int64))
    with pytest.raises(ValueError, match="out"):
        Q.toeplitz_hash_block_device(keys, seed, out[:4].reshape(2, 2))
    # a workspace allocated by the wrapper is freed on return: it cannot be kept for a raw stream handle
    with pytest.raises(ValueError, match="raw stream handle"):
        Q.toeplitz_hash_block_device(keys, seed, out[:4], stream=12345)
    Q.toeplitz_hash_block_device(keys, seed, out[:4], frames=torch.zeros(0, dtype=torch.int32))  # empty list: no call


def test_an_empty_list_touches_no_device():
    """n_list == 0 returns before any device call: it passes on a machine without one."""
    keys, seed = np.ones((3, 10), np.uint8), np.ones(40, np.uint8)
    out = Q.toeplitz_hash_block(keys, seed, 4, frames=[])
    assert out.dtype == np.uint8 and out.tolist() == [0, 0, 0, 0]
    assert Q.toeplitz_hash_block(np.zeros((0, 10), np.uint8), seed, 4).tolist() == [0, 0, 0, 0]
    assert privacy.block_tag(keys, seed, [], 8).tolist() == [0] * 8


# ---- lengths -------------------------------------------------------------------------------------
def test_block_secret_length_by_hand():
    # h2(1/4) = 0.8112781244...: 3 frames of 1000 bits keep 566.16...; less 0 + 100 + 104 leaked, 64 and 20
    got = privacy.block_secret_length(1000, [0, 100, 104, 5000], [0, 1, 2], 0.25, 64, 20)
    assert isinstance(got, int) and got == 278  # 566.16 - 204 - 84 = 278.16
    # one frame is secret_length's figure; the tag and the margin are paid once for the block
    per = privacy.secret_length(1000, [0, 100, 104], 0.25, 64, 20)
    assert privacy.block_secret_length(1000, [0, 100, 104], [1], 0.25, 64, 20) == per[1] == 4
    assert got > per.sum() + 84  # (three tags and margins against one, and the fractions add up)
    # list order does not matter, repeats count twice, and far below zero is zero
    assert privacy.block_secret_length(1000, [0, 100, 104, 5000], [2, 0, 1], 0.25, 64, 20) == 278
    assert privacy.block_secret_length(1000, [0, 100], [1, 1], 0.25, 64, 20) == 93  # 377.44 - 200 - 84
    assert privacy.block_secret_length(1000, [0, 100, 104, 5000], [0, 3], 0.25, 64, 20) == 0
    assert privacy.block_secret_length(1000, [0], [], 0.0, 0, 0) == 0
    assert privacy.block_secret_length(1000, [0, 16], [0, 1], 0.0, 64, 20) == 1900
