"""numpy's Toeplitz hash of one long block, independent of the kernel: the
index formula of include/qkd_ldpc_hip.h

    y[i] = XOR over j in [0, L) of  s[i + L - 1 - j] & x[j]

as entry i + L - 1 of the linear convolution of s and x, taken with a float64
real FFT of length N (the smallest power of two >= L + r - 1: the wrapped terms
of the cyclic convolution stay below index L - 1).  Every entry is an integer
<= L, so the rounding is checked: the largest distance to an integer must stay
below 0.25.  `toeplitz_at` evaluates the formula directly at chosen outputs and
pins the FFT (or the device) at sizes too large for toeplitz_ref.py."""
import numpy as np


def block_of(keys, frames, key_len):
    """The block: bit 0 of rows frames[0], frames[1], ... (None: every row) of keys, each cut to key_len."""
    k = np.asarray(keys, np.uint8)
    if k.ndim == 1:
        k = k[None, :]
    rows = k if frames is None else k[np.asarray(frames, np.int64)]
    return np.ascontiguousarray(rows[:, :key_len] & 1).reshape(-1)


def toeplitz_block_ref(x, s, r):
    """uint8 [r] from the block x [L] and the seed s [>= L + r - 1]; only bit 0 of a byte counts."""
    x = np.asarray(x, np.uint8).reshape(-1) & 1
    L = x.size
    s = np.asarray(s, np.uint8).reshape(-1)
    assert L >= 1 and r >= 1 and s.size >= L + r - 1
    s = s[:L + r - 1] & 1
    N = 1
    while N < L + r - 1:
        N *= 2
    if N == 1:
        return (x & s)[:1].copy()
    conv = np.fft.irfft(np.fft.rfft(x.astype(np.float64), N) * np.fft.rfft(s.astype(np.float64), N), N)[L - 1:L + r - 1]
    counts = np.rint(conv)
    assert np.abs(conv - counts).max() < 0.25, "the float64 convolution is not an integer any more"
    return (counts.astype(np.int64) & 1).astype(np.uint8)


def toeplitz_at(x, s, idx):
    """The formula itself at the outputs idx: uint8 [len(idx)]."""
    x = np.asarray(x, np.uint8).reshape(-1) & 1
    s = np.asarray(s, np.uint8).reshape(-1)
    L = x.size
    return np.array([np.count_nonzero(s[i:i + L][::-1] & x) & 1 for i in idx], np.uint8)
