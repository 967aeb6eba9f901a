"""A restatement of the error estimate at the reconciliation stage
(include/qkd_ldpc_hip.h, "Error estimation at the reconciliation stage") in
numpy and Python floats, with no import from the package.

H is a dense uint8 [m, n] matrix; punct / short are position lists (None or
empty: no plan).  Every float operation below is one IEEE-754 binary64 add,
subtract, multiply, compare or (log_p only) divide, in the order the header
fixes, so the product's doubles are compared bit for bit.
"""
import math

import numpy as np


def dense(H):
    """uint8 [m, n] from anything with n, m, row_ptr, col_idx."""
    D = np.zeros((H.m, H.n), np.uint8)
    for j in range(H.m):
        D[j, H.col_idx[H.row_ptr[j]:H.row_ptr[j + 1]]] = 1
    return D


def _lists(n, punct, short):
    p = np.asarray([] if punct is None else punct, np.int64).reshape(-1)
    s = np.asarray([] if short is None else short, np.int64).reshape(-1)
    keypos = np.setdiff1d(np.arange(n), np.concatenate([p, s]))
    return p, s, keypos


def row_degrees(D, punct=None, short=None):
    """int [m]: the effective degree of every informative row, 0 elsewhere."""
    p, s, _ = _lists(D.shape[1], punct, short)
    d = D.sum(axis=1, dtype=np.int64) - D[:, s].sum(axis=1, dtype=np.int64)
    d[D[:, p].sum(axis=1, dtype=np.int64) > 0] = 0
    return d


def classes(D, punct=None, short=None):
    """(degrees ascending, row counts) of the informative rows."""
    d = row_degrees(D, punct, short)
    deg, cnt = np.unique(d[d > 0], return_counts=True)
    return deg.astype(np.int64), cnt.astype(np.int64)


def extend(keys, n, punct=None, short=None):
    """Bob's extended key: key bits (bit 0 of each byte) at the key positions, 0 elsewhere."""
    keys = np.asarray(keys)
    _, _, keypos = _lists(n, punct, short)
    ext = np.zeros((keys.shape[0], n), np.uint8)
    ext[:, keypos] = keys[:, :keypos.size] & 1
    return ext


def weights(D, keys, synd, punct=None, short=None):
    """K_f: the informative rows at which the received syndrome differs from H * x~_f."""
    ext = extend(keys, D.shape[1], punct, short)
    hx = (ext.astype(np.float32) @ D.T.astype(np.float32)).astype(np.int64)  # (row counts < 2^24: exact)
    z = (hx & 1) ^ (np.asarray(synd).astype(np.int64) & 1)
    return z[:, row_degrees(D, punct, short) > 0].sum(axis=1).astype(np.int64)


def row_degrees_csr(H, punct=None, short=None):
    """row_degrees for a matrix too large to hold densely (n, m, row_ptr, col_idx)."""
    p, s, _ = _lists(H.n, punct, short)
    cls = np.zeros(H.n, np.int64)
    cls[p], cls[s] = 1, 2
    c = cls[np.asarray(H.col_idx, np.int64)]
    rp = np.asarray(H.row_ptr, np.int64)
    per_row = lambda v: np.diff(np.concatenate([[0], np.cumsum(v)])[rp])
    d = per_row(np.ones(c.size, np.int64)) - per_row(c == 2)
    d[per_row(c == 1) > 0] = 0
    return d


def weights_csr(H, keys, synd, punct=None, short=None):
    """weights for a matrix too large to hold densely: row parities from prefix sums."""
    ext = extend(keys, H.n, punct, short).astype(np.int64)
    rp = np.asarray(H.row_ptr, np.int64)
    pre = np.concatenate([np.zeros((ext.shape[0], 1), np.int64), np.cumsum(ext[:, np.asarray(H.col_idx)], axis=1)], axis=1)
    z = ((pre[:, rp[1:]] - pre[:, rp[:-1]]) & 1) ^ (np.asarray(synd).astype(np.int64) & 1)
    return z[:, row_degrees_csr(H, punct, short) > 0].sum(axis=1).astype(np.int64)


def expected_weight(deg, cnt, q):
    t = 1.0 - 2.0 * q
    pw, acc, d = 1.0, 0.0, 0
    for dc, nc in zip(deg, cnt):
        while d < int(dc):
            pw = pw * t
            d += 1
        acc = acc + float(int(nc)) * (0.5 * (1.0 - pw))
    return acc


def qber(deg, cnt, weight, q_min, q_max, frames=1):
    k, f = float(int(weight)), float(int(frames))
    if f * expected_weight(deg, cnt, q_min) >= k:
        return q_min
    if f * expected_weight(deg, cnt, q_max) <= k:
        return q_max
    lo, hi = q_min, q_max
    for _ in range(64):
        mid = 0.5 * (lo + hi)
        if mid == lo or mid == hi:
            break
        if f * expected_weight(deg, cnt, mid) < k:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


def log_p(q):
    return math.log1p((1.0 - 2.0 * q) / q)


def estimate(D, keys, synd, punct=None, short=None, q_min=1e-4, q_max=0.25):
    """(qber float64, log_p float64, weight int64), one per frame."""
    deg, cnt = classes(D, punct, short)
    w = weights(D, keys, synd, punct, short)
    q = np.array([qber(deg, cnt, k, q_min, q_max) for k in w], np.float64)
    return q, np.array([log_p(x) for x in q], np.float64), w


def corrected_errors(keys, bits, punct=None, short=None):
    """E_f: key positions at which the key differs from the decoded frame."""
    bits = np.asarray(bits)
    _, _, keypos = _lists(bits.shape[1], punct, short)
    return ((np.asarray(keys)[:, :keypos.size] ^ bits[:, keypos]) & 1).sum(axis=1).astype(np.int64)
