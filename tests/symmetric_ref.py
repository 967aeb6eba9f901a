"""Symmetric blind reconciliation restated with numpy and the CPU oracle: the
selection order, and the whole exchange with the oracle decoding each round's
pinned LLRs (the counterpart of test_gpu_blind.np_blind)."""
import sys

import numpy as np

DBL_MAX = sys.float_info.max
MAG = np.uint64(0x7FFFFFFFFFFFFFFF)


def np_select(post_row, excluded_mask, count):
    """The `count` positions of post_row that are not excluded, smallest first
    under (the posterior's 64 bits with the sign cleared, index)."""
    post_row = np.ascontiguousarray(post_row, np.float64)
    u = post_row.view(np.uint64) & MAG
    idx = np.arange(post_row.size)
    cand = np.flatnonzero(~np.asarray(excluded_mask, bool))
    order = np.lexsort((idx[cand], u[cand]))  # (the last key is the primary one)
    assert count <= cand.size
    return cand[order[:count]].astype(np.int32)


def excluded(n, short=None, history=()):
    m = np.zeros(n, bool)
    if short is not None:
        m[np.asarray(short, np.int64)] = True
    m[np.asarray(history, np.int64)] = True
    return m


def pinned_positions_llr(llr0, ext, frames, positions, n_disc):
    """Bob's LLRs of the listed frames with positions[f, :n_disc] pinned at
    Alice's bits there: bit ? -DBL_MAX : +DBL_MAX, whatever the position's class."""
    llr = llr0[frames].copy()
    for j, f in enumerate(frames):
        p = positions[f, :n_disc].astype(np.int64)
        llr[j, p] = np.where(ext[f, p] & 1, -DBL_MAX, DBL_MAX)
    return llr


def np_symmetric(oracle, oparams, llr0, syn, ext, short=None, step=20, max_rounds=None, max_disclosed=None):
    """The exchange -> (states after rounds 0, 1, ... as (bits, iterations, ok,
    posterior); the failed lists of rounds 1, ...; per frame the round, the
    disclosed count, the summed iterations; positions [batch, cap], -1 filled)."""
    batch, n = llr0.shape
    n_short = 0 if short is None else len(short)
    cap = n - n_short if max_disclosed is None else min(max_disclosed, n - n_short)
    if max_rounds is not None:
        cap = min(cap, step * max_rounds)
    st = oracle.decode_batch(oparams, llr0, syn, threads=8, posterior=True)
    states, lists = [st], []
    rounds, disclosed = np.zeros(batch, np.int32), np.zeros(batch, np.int32)
    iters = st[1].astype(np.uint32)
    positions = np.full((batch, max(cap, 1)), -1, np.int32)
    r = d = 0
    while d < cap and (max_rounds is None or r < max_rounds):
        failed = np.flatnonzero(st[2] == 0)
        if failed.size == 0:
            break
        r, c = r + 1, min(step, cap - d)
        for f in failed:
            positions[f, d:d + c] = np_select(st[3][f], excluded(n, short, positions[f, :d]), c)
        d += c
        res = oracle.decode_batch(oparams, pinned_positions_llr(llr0, ext, failed, positions, d), syn[failed],
                                  threads=8, posterior=True)
        st = tuple(x.copy() for x in st)
        for o, x in zip(st, res):
            o[failed] = x
        iters[failed] += res[1].astype(np.uint32)
        rounds[failed], disclosed[failed] = r, d
        states.append(st)
        lists.append(failed)
    return states, lists, rounds, disclosed, iters, positions
