"""numpy's Toeplitz hash, written from the index formula of
include/qkd_ldpc_hip.h and not from the kernel's word layout:

    y[i] = XOR over j in [0, L) of  s[i + L - 1 - j] & x[j]

sliding_window_view over the seed gives the rows s[i .. i + L) of the matrix
read right to left, so the keys are reversed to match and the rest is a sum
mod 2 (a float32 matmul: exact while L < 2^24)."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view


def toeplitz_ref(keys, seed, out_len, key_len=None):
    """uint8 [batch, out_len] from keys [batch, >= key_len] and seed
    [>= key_len + out_len - 1]; only bit 0 of a byte counts."""
    k = np.asarray(keys, np.uint8)
    if k.ndim == 1:
        k = k[None, :]
    L = k.shape[1] if key_len is None else int(key_len)
    assert 1 <= L <= k.shape[1] and L < (1 << 24) and out_len >= 1
    s = np.asarray(seed, np.uint8).reshape(-1)
    assert s.size >= L + out_len - 1
    s = s[:L + out_len - 1] & 1
    xr = np.ascontiguousarray((k[:, :L] & 1)[:, ::-1].T).astype(np.float32)  # [L, batch], xr[u] = x[L - 1 - u]
    win = sliding_window_view(s, L)  # win[i][u] = s[i + u]
    out = np.empty((k.shape[0], out_len), np.uint8)
    for i0 in range(0, out_len, 512):
        rows = win[i0:i0 + 512].astype(np.float32)
        out[:, i0:i0 + 512] = ((rows @ xr).astype(np.int64) & 1).T
    return out


def cut(full, lens):
    """Row f of `full` up to lens[f], zeros after."""
    full = np.asarray(full, np.uint8)
    keep = np.arange(full.shape[1])[None, :] < np.asarray(lens)[:, None]
    return np.where(keep, full, 0).astype(np.uint8)
