"""Where the QBER comes from: error estimation at the reconciliation stage
(Kiktenko et al., arXiv:1810.05841) over Graph.estimate_qber and
Graph.corrected_errors.  Bob computes all of it alone: nothing here needs the
channel.

Before the decode Bob compares the syndrome he received with the syndrome of
his own key: the weight of the difference over the informative check rows
gives q, and with it the log_p the decode starts from (`prior`).  After the
decode a frame that verified tells him its error count exactly
(`corrected_errors`); summed over a verified block that is the q the secret
length is computed from (`block_qber`), and an exponential moving average
carries it to the next batch (`Tracker`).
"""
from __future__ import annotations

import numpy as np

__all__ = ["prior", "corrected_errors", "block_qber", "Tracker"]


def prior(gb, bob_keys: np.ndarray, syndrome: np.ndarray, plan=None, q_min: float = 1e-4, q_max: float = 0.25,
          pooled: bool = False):
    """Bob's estimate before the decode: (qber float64, log_p float64, weight
    int32), [batch] each.  log_p is what Graph.reconcile, blind.blind_reconcile
    and blind.symmetric_reconcile take as their log_p.  pooled: one estimate
    from the sum of the batch's weights, given to every frame (frames that
    share a channel); otherwise one estimate per frame."""
    q, lp, w = gb.estimate_qber(bob_keys, syndrome, plan=plan, q_min=q_min, q_max=q_max)
    if pooled and w.size:
        q1, lp1 = gb.qber_from_weight([int(w.sum(dtype=np.int64))], plan=plan, q_min=q_min, q_max=q_max,
                                      frames_per_weight=int(w.size))
        q, lp = np.full(w.size, q1[0]), np.full(w.size, lp1[0])
    return q, lp, w


def corrected_errors(gb, bob_keys: np.ndarray, bits: np.ndarray, plan=None) -> np.ndarray:
    """int32 [batch]: the key positions at which Bob's key differs from the
    decoded frame (punctured and shortened positions do not count).  A frame's
    exact error count only when the frame verified."""
    return gb.corrected_errors(bob_keys, bits, plan=plan)


def block_qber(errors, n_key: int, frames) -> float:
    """sum of errors[frames] / (len(frames) * n_key): the measured QBER of a
    verified block, the q to pass to privacy.block_secret_length.  0.0 for an
    empty list."""
    fr = np.asarray(frames, np.int64).reshape(-1)
    if fr.size == 0:
        return 0.0
    e = np.asarray(errors, np.int64).reshape(-1)
    return int(e[fr].sum()) / (fr.size * int(n_key))


class Tracker:
    """The running estimate of arXiv:1810.05841: q <- alpha q_measured +
    (1 - alpha) q after every verified block.  It carries a block's
    `block_qber` to the next batch's [q_min, q_max] window or rate choice."""

    def __init__(self, alpha: float, q0: float):
        if not 0.0 <= alpha <= 1.0:
            raise ValueError("alpha must be in [0, 1]")
        self.alpha, self.q = float(alpha), float(q0)

    def update(self, q_measured: float) -> float:
        self.q = self.alpha * float(q_measured) + (1.0 - self.alpha) * self.q
        return self.q
