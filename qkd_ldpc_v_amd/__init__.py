"""qkd_ldpc_v_amd — MI355X (gfx950) LDPC belief-propagation decoding for QKD.

The product is libqkdldpc_hip.so (HIP kernels + C ABI, include/qkd_ldpc_hip.h);
this package binds it and mirrors the reference's decode interface
(ColdCloudd/QKD_LDPC_V src/qkd_ldpc_algorithm.hpp).

Two parties: Alice publishes Graph.syndrome(keys[, plan, punct_fill]); Bob
decodes with Graph.reconcile(params, keys, log_p, syndrome[, plan]) from his own
key and the received syndrome (device forms: syndrome_device, reconcile_device,
extract_key_device).  Neither call sees the other side's key.

Frames that fail are decoded again in disclosure rounds (blind reconciliation):
blind.blind_reconcile runs the exchange over Graph.failed_frames_device,
Graph.disclose[_device] (Alice) and Graph.reconcile_round[_device] (Bob).
blind.symmetric_reconcile discloses each frame's least reliable positions
instead (Graph.select_positions, disclose_positions, reconcile_positions_round,
each with a _device form); it needs no rate plan.

Both sides then hash their keys (toeplitz_hash[_device], a Toeplitz hash over
GF(2)): privacy.tag / privacy.verified compare a short tag per frame, and
privacy.amplify shortens the verified frames by what the exchange leaked
(privacy.leaked_bits, privacy.secret_length).  toeplitz_hash_block[_device]
hashes the concatenation of a list of frames' keys as one block, up to 2^27
bits (privacy.block_tag, privacy.block_secret_length, privacy.block_amplify).

The QBER those steps take comes from the exchange itself (estimate.py):
estimate.prior gives Bob's log_p before the decode from the syndrome weight
(Graph.estimate_qber[_device], Graph.estimate_classes, Graph.qber_from_weight),
estimate.corrected_errors and estimate.block_qber the measured QBER of the
verified frames after it (Graph.corrected_errors[_device]).
"""
from ._lib import (ALGORITHM_NAMES, ANMSA, AOMSA, NMSA, OMSA, SPA, SPA_LIN, SELECT_MAX, TRACE_NONE, Params, QLDPCError,
                   exported_symbols, lib, log_p, version)
from .graph import (DecodeOutput, Graph, HMatrix, RatePlan, TraceOutput, TrialsOutput, adapt_code_rate, keys_match_device, load_matrix,
                    select_punctured_untainted, toeplitz_block_workspace, toeplitz_hash, toeplitz_hash_block,
                    toeplitz_hash_block_device, toeplitz_hash_device,
                    trial_seeds, trials_device, trials_rate_adapt_device, xoshiro_state)
from .trials import bsc_frames
from .codes import regular_code
from . import blind, estimate, privacy
from .blind import BlindOutput, SymmetricOutput, blind_efficiency, blind_reconcile, symmetric_reconcile

__all__ = [
    "regular_code",
    "ALGORITHM_NAMES", "ANMSA", "AOMSA", "NMSA", "OMSA", "SPA", "SPA_LIN", "Params", "QLDPCError",
    "exported_symbols", "lib", "log_p", "version", "DecodeOutput", "TrialsOutput", "Graph", "HMatrix", "keys_match_device",
    "trial_seeds", "trials_device", "RatePlan", "adapt_code_rate", "trials_rate_adapt_device", "xoshiro_state",
    "load_matrix", "bsc_frames", "TraceOutput", "TRACE_NONE", "blind", "BlindOutput", "blind_efficiency",
    "blind_reconcile", "SymmetricOutput", "symmetric_reconcile", "SELECT_MAX", "privacy", "toeplitz_hash", "toeplitz_hash_device",
    "toeplitz_block_workspace", "toeplitz_hash_block", "toeplitz_hash_block_device", "estimate",
]
