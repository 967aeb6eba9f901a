"""Key verification and privacy amplification over the batched Toeplitz hash
(toeplitz_hash, qldpc_toeplitz_hash_batch).

After reconciliation each side holds n_key bits per frame.  Both hash them
under one public seed to a short tag; frames whose tags differ are dropped
(`tag`, `verified`).  The verified frames are hashed again, under a second
seed, to a length that takes out what the exchange leaked (`leaked_bits`,
`secret_length`, `amplify`).  Seeds are public and shared; how they are drawn
and how the channel is authenticated is the caller's.

Blocks: `block_tag`, `block_secret_length` and `block_amplify` do the same for
the concatenation of a list of frames' keys hashed as one key
(toeplitz_hash_block): one tag, one leak sum and one margin per block, and a
key long enough for a finite-key bound to be worth applying.
"""
from __future__ import annotations

import numpy as np

from .blind import h2, leaked_bits
from .graph import toeplitz_hash, toeplitz_hash_block

__all__ = ["tag", "verified", "leaked_bits", "secret_length", "amplify", "block_tag", "block_secret_length",
           "block_amplify"]


def tag(keys: np.ndarray, seed: np.ndarray, tag_bits: int = 64) -> np.ndarray:
    """The verification tag of every key row: the hash with out_len = tag_bits,
    uint8 [batch, tag_bits].  seed holds row length + tag_bits - 1 entries."""
    return toeplitz_hash(keys, seed, tag_bits)


def verified(tag_a: np.ndarray, tag_b: np.ndarray) -> np.ndarray:
    """uint8 [batch]: 1 where the two sides' tags agree."""
    a, b = np.asarray(tag_a), np.asarray(tag_b)
    if a.shape != b.shape or a.ndim != 2:
        raise ValueError(f"tags of shapes {a.shape} and {b.shape}")
    return (a == b).all(axis=1).astype(np.uint8)


def secret_length(n_key: int, leaked, q: float, tag_bits: int, security_bits: int) -> np.ndarray:
    """max(0, floor(n_key (1 - h2(q)) - leaked - tag_bits - security_bits)) per
    frame, int32.  This is the asymptotic BB84 figure — the phase-error term
    n_key h2(q) at the estimated QBER q, the reconciliation leak, the published
    tag and a fixed margin — and NOT a finite-key bound: callers with a bound of
    their own pass their own lengths to `amplify`."""
    lk = np.asarray(leaked, np.float64)
    length = np.floor(n_key * (1.0 - h2(float(q))) - lk - tag_bits - security_bits)
    return np.maximum(length, 0.0).astype(np.int32)


def amplify(keys: np.ndarray, seed: np.ndarray, lengths):
    """Privacy amplification: row f of the result is the first lengths[f] bits
    of the hash of keys[f], then zeros, uint8 [batch, max(lengths)]; returned
    with the lengths (int32).  A frame of length 0 (failed or unverified) comes
    back all zero.  seed holds at least row length + max(lengths) - 1 entries."""
    lens = np.ascontiguousarray(lengths, np.int32).reshape(-1)
    k = np.asarray(keys)
    batch = 1 if k.ndim == 1 else k.shape[0]
    if lens.size != batch:
        raise ValueError(f"expected {batch} lengths")
    if lens.size and int(lens.min()) < 0:
        raise ValueError("lengths must be >= 0")
    width = int(lens.max()) if lens.size else 0
    if width == 0:
        return np.zeros((batch, 0), np.uint8), lens
    return toeplitz_hash(k, seed, width, out_lens=lens), lens


def block_tag(keys: np.ndarray, seed: np.ndarray, frames, tag_bits: int = 64) -> np.ndarray:
    """The verification tag of the block keys[frames[0]] | keys[frames[1]] | ...:
    uint8 [tag_bits].  seed holds len(frames) * row length + tag_bits - 1 entries."""
    return toeplitz_hash_block(keys, seed, tag_bits, frames=frames)


def block_secret_length(n_key: int, leaked, frames, q: float, tag_bits: int, security_bits: int) -> int:
    """max(0, floor(n_list n_key (1 - h2(q)) - sum of leaked[frames] - tag_bits -
    security_bits)) for the block of the listed frames (n_list = len(frames)):
    the asymptotic figure of `secret_length`, with the tag and the margin paid
    once per block instead of once per frame.  It is still NOT a finite-key
    bound — that remains the caller's, who passes a length of their own to
    `block_amplify`; what a block gives them is a key long enough for the
    statistical terms of such a bound, which fall like 1 / sqrt(block length),
    to leave something."""
    fr = np.asarray(frames, np.int64).reshape(-1)
    lk = np.asarray(leaked, np.float64).reshape(-1)
    length = np.floor(fr.size * n_key * (1.0 - h2(float(q))) - float(lk[fr].sum()) - tag_bits - security_bits)
    return max(0, int(length))


def block_amplify(keys: np.ndarray, seed: np.ndarray, frames, length: int) -> np.ndarray:
    """Privacy amplification of a block: the first `length` bits of the hash of
    keys[frames[0]] | keys[frames[1]] | ..., uint8 [length] (length 0: nothing to
    hash, an empty array).  seed holds at least len(frames) * row length +
    length - 1 entries."""
    length = int(length)
    if length < 0:
        raise ValueError("length must be >= 0")
    if length == 0:
        return np.zeros(0, np.uint8)
    return toeplitz_hash_block(keys, seed, length, frames=frames)
