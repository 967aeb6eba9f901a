"""Blind reconciliation (Martinez-Mateo, Elkouss, Martin, arXiv:1205.5729) over
the two-party entries: frames whose decode failed are decoded again after Alice
has disclosed some of her punctured bits, round after round, under one rate
plan and one syndrome.

Per round, Bob -> Alice: the list of frames that failed; Alice -> Bob: the
values of the next `step` punctured bits of those frames.  Each disclosed bit
is a leaked bit, which `efficiency` accounts for.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

from ._lib import Params
from .graph import Graph, RatePlan


@dataclass
class BlindOutput:
    bits: np.ndarray        # uint8[batch, n]  Bob's extended frames after the frame's last round
    synd_ok: np.ndarray     # uint8[batch]     syndromes_match of the frame's last round
    rounds: np.ndarray      # int32[batch]     the round the frame decoded in (0: one-shot), or the last round run
    disclosed: np.ndarray   # int32[batch]     punctured bits Alice disclosed for the frame
    iterations: np.ndarray  # uint32[batch]    decoder iterations, summed over the frame's rounds
    efficiency: np.ndarray  # float64[batch]   blind_efficiency of the frame (NaN without q)


@dataclass
class SymmetricOutput(BlindOutput):
    """symmetric_reconcile's result: `disclosed` counts positions of any class."""
    positions: np.ndarray = None  # int32[batch, cap]  the positions disclosed for the frame, in order; -1 past disclosed[f]


def h2(q: float) -> float:
    """The binary entropy, in bits."""
    if q <= 0.0 or q >= 1.0:
        return 0.0
    return -q * math.log2(q) - (1.0 - q) * math.log2(1.0 - q)


def leaked_bits(n: int, m: int, n_punct: int, n_short: int, disclosed):
    """m - n_punct + disclosed: the bits the exchange revealed about a frame's
    key — syndrome bits that are not spent on punctured positions, plus the
    punctured bits Alice disclosed.  What privacy amplification must remove."""
    return (m - n_punct) + np.asarray(disclosed)


def blind_efficiency(n: int, m: int, n_punct: int, n_short: int, disclosed, q: float | None):
    """leaked_bits / ((n - n_punct - n_short) h2(q)): the bits the exchange
    revealed about a frame's key over the Slepian-Wolf bound for its
    n - n_punct - n_short key bits.  NaN when q is not given."""
    d = np.asarray(disclosed, np.float64)
    if q is None:
        return np.full(d.shape, np.nan)
    return leaked_bits(n, m, n_punct, n_short, d) / ((n - n_punct - n_short) * h2(float(q)))


def check_order(order, n_punct: int) -> np.ndarray:
    """`order` as int32 indices into the plan's punctured list; it must be a
    permutation of range(n_punct) (None: ascending)."""
    if order is None:
        return np.arange(n_punct, dtype=np.int32)
    o = np.asarray(order)
    if o.ndim != 1 or o.size != n_punct or not np.issubdtype(o.dtype, np.integer) or \
            not np.array_equal(np.sort(o), np.arange(n_punct)):
        raise ValueError(f"order must be a permutation of range({n_punct})")
    return np.ascontiguousarray(o, np.int32)


def failed_frames(graph: Graph, synd_ok: np.ndarray) -> np.ndarray:
    """The frames with synd_ok == 0, ascending, listed on the device."""
    import torch

    ok = np.ascontiguousarray(synd_ok, np.uint8)
    if ok.size == 0:
        return np.empty(0, np.int32)
    d_ok = torch.from_numpy(ok).cuda()
    d_list = torch.empty(ok.size, dtype=torch.int32, device="cuda")
    d_count = torch.zeros(1, dtype=torch.int32, device="cuda")
    graph.failed_frames_device(d_ok, d_list, d_count)
    count = int(d_count.cpu()[0])  # (the four bytes Bob reads between rounds)
    return d_list[:count].cpu().numpy()


def blind_reconcile(ga: Graph, plan_a: RatePlan, gb: Graph, plan_b: RatePlan, params: Params, alice: np.ndarray,
                    bob: np.ndarray, log_p, fill: np.ndarray, step: int, order=None, max_rounds: int | None = None,
                    q: float | None = None) -> BlindOutput:
    """The whole exchange for a batch.  Alice (ga, plan_a, her keys and private
    fill) publishes one syndrome per frame; Bob (gb, plan_b, his keys) decodes
    (round 0) and then, while frames fail and punctured bits remain, names the
    failed frames, receives the next `step` bits of `order` for them and decodes
    them again with every bit received so far pinned.  max_rounds bounds the
    disclosure rounds (None: until nothing is left to disclose)."""
    n_punct = int(plan_b.punctured.size)
    if int(plan_a.punctured.size) != n_punct or not np.array_equal(plan_a.punctured, plan_b.punctured) or \
            not np.array_equal(plan_a.shortened, plan_b.shortened):
        raise ValueError("Alice's and Bob's plans differ")
    if step < 1:
        raise ValueError("step must be >= 1")
    order = check_order(order, n_punct)
    fill = np.ascontiguousarray(fill, np.uint8).reshape(-1, max(n_punct, 1))

    _, syndrome = ga.syndrome(alice, plan_a, fill if n_punct else None)  # Alice -> Bob, once
    out = gb.reconcile(params, bob, log_p, syndrome, plan=plan_b)
    batch = out.synd_ok.shape[0]
    rounds = np.zeros(batch, np.int32)
    disclosed = np.zeros(batch, np.int32)
    iterations = out.iterations.astype(np.uint32)
    known = np.zeros((batch, max(n_punct, 1)), np.uint8)  # Bob's record of the bits he received
    r = d = 0
    while d < n_punct and (max_rounds is None or r < max_rounds):
        failed = failed_frames(gb, out.synd_ok)  # Bob -> Alice
        if failed.size == 0:
            break
        r += 1
        new = order[d:min(d + step, n_punct)]
        d += new.size
        known[np.ix_(failed, new)] = ga.disclose(plan_a, failed, fill, new)  # Alice -> Bob
        gb.reconcile_round(params, bob, log_p, syndrome, plan_b, failed, order[:d], known[np.ix_(failed, order[:d])],
                           out=out)  # (rows `failed` of out: this round's decode)
        iterations[failed] += out.iterations[failed]
        rounds[failed] = r
        disclosed[failed] = d
    eff = blind_efficiency(gb.n, gb.m, n_punct, int(plan_b.shortened.size), disclosed, q)
    return BlindOutput(out.bits, out.synd_ok, rounds, disclosed, iterations, eff)


def symmetric_reconcile(ga: Graph, plan_a: RatePlan | None, gb: Graph, plan_b: RatePlan | None, params: Params,
                        alice_keys: np.ndarray, bob_keys: np.ndarray, lp, punct_fill: np.ndarray | None = None,
                        step: int = 20, max_rounds: int | None = None, max_disclosed: int | None = None,
                        q: float | None = None) -> SymmetricOutput:
    """Symmetric blind reconciliation (Kiktenko et al., arXiv:1612.03673) for a
    batch.  Round 0 is Bob's decode against Alice's syndrome, with the posterior
    kept.  While frames fail, Bob picks for each the `step` candidate positions
    of smallest |posterior| (select_positions) and names them to Alice with the
    failed list, Alice answers with her bits there (disclose_positions), and Bob
    decodes those frames again with every position received so far pinned
    (reconcile_positions_round).  It ends when nothing fails, after max_rounds
    disclosure rounds, or at max_disclosed positions per frame (None: every
    candidate, n - shortened).  The plans may be None on both sides: then every
    position is a key position and a disclosed bit is a key bit.  Disclosed key
    positions stay in the key; leaked_bits counts them for privacy amplification."""
    if (plan_a is None) != (plan_b is None):
        raise ValueError("Alice's and Bob's plans differ")
    n_punct = n_short = 0
    if plan_b is not None:
        n_punct, n_short = int(plan_b.punctured.size), int(plan_b.shortened.size)
        if not np.array_equal(plan_a.punctured, plan_b.punctured) or \
                not np.array_equal(plan_a.shortened, plan_b.shortened):
            raise ValueError("Alice's and Bob's plans differ")
    if step < 1:
        raise ValueError("step must be >= 1")
    cap = gb.n - n_short if max_disclosed is None else min(int(max_disclosed), gb.n - n_short)
    if cap < 0:
        raise ValueError("max_disclosed must be >= 0")
    if max_rounds is not None:
        cap = min(cap, step * max(int(max_rounds), 0))

    if plan_a is None:  # Alice -> Bob, once
        syndrome = ga.syndrome(alice_keys)
        ext = np.ascontiguousarray(alice_keys, np.uint8).reshape(-1, ga.n)
    else:
        fill = None if not n_punct else np.ascontiguousarray(punct_fill, np.uint8).reshape(-1, n_punct)
        ext, syndrome = ga.syndrome(alice_keys, plan_a, fill)
    out = gb.reconcile(params, bob_keys, lp, syndrome, plan=plan_b, posterior=True)
    batch = out.synd_ok.shape[0]
    rounds = np.zeros(batch, np.int32)
    disclosed = np.zeros(batch, np.int32)
    iterations = out.iterations.astype(np.uint32)
    positions = np.full((batch, max(cap, 1)), -1, np.int32)
    known = np.zeros((batch, max(cap, 1)), np.uint8)  # Bob's record of the bits he received
    r = d = 0
    while d < cap and (max_rounds is None or r < max_rounds):
        failed = failed_frames(gb, out.synd_ok)
        if failed.size == 0:
            break
        r += 1
        c = min(step, cap - d)
        gb.select_positions(out.posterior, failed, d, c, positions, plan=plan_b)  # Bob -> Alice, with the list
        known[failed, d:d + c] = ga.disclose_positions(ext, failed, positions, d, c, plan=plan_a)  # Alice -> Bob
        d += c
        gb.reconcile_positions_round(params, bob_keys, lp, syndrome, failed, d, positions, known[failed, :d],
                                     plan=plan_b, out=out)  # (rows `failed` of out: this round's decode and posterior)
        iterations[failed] += out.iterations[failed]
        rounds[failed] = r
        disclosed[failed] = d
    eff = blind_efficiency(gb.n, gb.m, n_punct, n_short, disclosed, q)
    return SymmetricOutput(out.bits, out.synd_ok, rounds, disclosed, iterations, eff, positions)
