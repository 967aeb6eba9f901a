"""Parity-check matrices and device graphs.

HMatrix mirrors the reference's H_matrix (src/array_and_matrix_operations.hpp:
60-77) as flat CSR (check_nodes) + CSC (bit_nodes) arrays; load_matrix() calls
the C ABI's reader, which restates the reference's four file formats.
Graph owns a qldpc_graph: the decoder's lane partition, replicated on devices.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

import numpy as np

from . import _lib
from ._lib import Params, check, lib, ptr


@dataclass
class HMatrix:
    n: int
    m: int
    row_ptr: np.ndarray  # int32[m+1] check_nodes
    col_idx: np.ndarray  # int32[nnz]
    col_ptr: np.ndarray  # int32[n+1] bit_nodes
    row_idx: np.ndarray  # int32[nnz]
    is_regular: bool = False

    @property
    def nnz(self) -> int:
        return int(self.row_ptr[-1])

    @property
    def check_nodes(self) -> list[list[int]]:
        rp, ci = self.row_ptr, self.col_idx
        return [ci[rp[j]:rp[j + 1]].tolist() for j in range(self.m)]

    @property
    def bit_nodes(self) -> list[list[int]]:
        cp, ri = self.col_ptr, self.row_idx
        return [ri[cp[i]:cp[i + 1]].tolist() for i in range(self.n)]

    @property
    def code_rate(self) -> float:
        """1 - M/N (reference src/simulation.cpp:389)."""
        return 1.0 - self.m / self.n

    @classmethod
    def from_check_nodes(cls, n: int, check_nodes: list[list[int]]) -> "HMatrix":
        """H from per-check bit lists; bit_nodes is the ascending transpose."""
        m = len(check_nodes)
        row_ptr = np.zeros(m + 1, np.int32)
        row_ptr[1:] = np.cumsum([len(r) for r in check_nodes])
        col_idx = np.array([c for r in check_nodes for c in r], np.int32)
        order = np.lexsort((np.repeat(np.arange(m), np.diff(row_ptr)), col_idx))
        row_idx = np.repeat(np.arange(m, dtype=np.int32), np.diff(row_ptr))[order]
        col_ptr = np.zeros(n + 1, np.int32)
        col_ptr[1:] = np.cumsum(np.bincount(col_idx, minlength=n))
        return cls(n, m, row_ptr, col_idx, col_ptr, row_idx.astype(np.int32), False)

    def syndrome(self, bits: np.ndarray) -> np.ndarray:
        """calculate_syndrome over the last axis (src/array_and_matrix_operations.cpp:936-950)."""
        b = np.asarray(bits, np.uint8)
        vals = b[..., self.col_idx].astype(np.int64)
        cs = np.concatenate([np.zeros(b.shape[:-1] + (1,), np.int64), np.cumsum(vals, axis=-1)], axis=-1)
        # (advanced indexing on the last axis yields a Fortran-ordered result: make it row-major)
        return np.ascontiguousarray(((cs[..., self.row_ptr[1:]] - cs[..., self.row_ptr[:-1]]) & 1).astype(np.uint8))


def load_matrix(path: str, fmt: int) -> HMatrix:
    """Read a matrix file in reference format `fmt` (0 uncompressed, 1 alist, 2 sparse_1, 3 sparse_2)."""
    L = lib()
    n, m, nnz, reg = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    p = str(path).encode()
    check(L.qldpc_load_matrix(p, fmt, ctypes.byref(n), ctypes.byref(m), ctypes.byref(nnz), None, None, None, None,
                              ctypes.byref(reg)), f"qldpc_load_matrix({path})")
    rp = np.empty(m.value + 1, np.int32)
    ci = np.empty(nnz.value, np.int32)
    cp = np.empty(n.value + 1, np.int32)
    ri = np.empty(nnz.value, np.int32)
    check(L.qldpc_load_matrix(p, fmt, ctypes.byref(n), ctypes.byref(m), ctypes.byref(nnz), ptr(rp), ptr(ci), ptr(cp),
                              ptr(ri), ctypes.byref(reg)), f"qldpc_load_matrix({path})")
    return HMatrix(n.value, m.value, rp, ci, cp, ri, bool(reg.value))


@dataclass
class DecodeOutput:
    bits: np.ndarray        # uint8[batch, n]  bit_array_out
    iterations: np.ndarray  # uint32[batch]    decoding_result.iterations_num
    synd_ok: np.ndarray     # uint8[batch]     decoding_result.syndromes_match
    posterior: np.ndarray | None  # float64[batch, n] total_bit_llr


@dataclass
class TraceOutput(DecodeOutput):
    """A decode and its per-iteration trace (qldpc_decode_trace_batch): row `it`
    of a frame exists when the bit pass of iteration `it` ran for it; the
    others read TRACE_NONE / NaN."""
    unsat: np.ndarray  # uint32[batch, max_it] checks off their syndrome bit after each bit pass
    trace_posterior: np.ndarray | None  # float64[batch, max_it, n] total_bit_llr after each bit pass

    @property
    def rows(self) -> np.ndarray:
        """Trace rows per frame."""
        return (self.unsat != _lib.TRACE_NONE).sum(axis=1)


@dataclass
class TrialsOutput:
    iterations: np.ndarray  # uint32[count] decoding_result.iterations_num
    synd_ok: np.ndarray     # uint8[count]  decoding_result.syndromes_match
    keys_match: np.ndarray  # uint8[count]  LDPC_result.keys_match
    runtime_us: np.ndarray  # float64[count] trial_result.runtime (share of the chunk window, see the C ABI)
    accurate_qber: float    # trial_result.accurate_QBER (the same for every trial)


class TrialsJob:
    """One combination's trials in flight (qldpc_run_trials_submit); keeps the
    graph, the rate plan and the output arrays alive until wait()."""

    def __init__(self, graph, plan, count: int):
        self.graph, self.plan, self.handle = graph, plan, None
        self.it = np.empty(count, np.uint32)
        self.ok = np.empty(count, np.uint8)
        self.km = np.empty(count, np.uint8)
        self.rt = np.empty(count, np.float64)
        self.q = ctypes.c_double(0.0)
        self._out = None

    def wait(self) -> TrialsOutput:
        if self._out is None:
            h, self.handle = self.handle, None
            check(lib().qldpc_run_trials_wait(h), "qldpc_run_trials_wait")
            self._out = TrialsOutput(self.it, self.ok, self.km, self.rt, self.q.value)
        return self._out

    def __del__(self):
        if self.handle is not None:  # a job is always completed (its slots hold our arrays)
            try:
                lib().qldpc_run_trials_wait(self.handle)
            except Exception:
                pass


def _canonical_adjacency(H: HMatrix) -> bool:
    """check_nodes rows ascending and bit_nodes their ascending transpose: the
    reference's slot pairing is then the edge itself (src/qkd_ldpc_algorithm.cpp:
    67-69,116-118)."""
    rp, ci = np.asarray(H.row_ptr), np.asarray(H.col_idx)
    rows = np.repeat(np.arange(H.m, dtype=np.int64), np.diff(rp))
    if ci.size and np.any((np.diff(ci) <= 0) & (rows[1:] == rows[:-1])):
        return False
    order = np.lexsort((rows, ci))
    cp = np.zeros(H.n + 1, np.int64)
    np.add.at(cp, ci.astype(np.int64) + 1, 1)
    return np.array_equal(np.cumsum(cp), np.asarray(H.col_ptr)) and np.array_equal(rows[order], np.asarray(H.row_idx))


class Graph:
    """A device-resident Tanner graph (qldpc_graph).

    device_mask: replicate on these HIP devices (bit d = device d; 0 = the
    current one).  devices: an explicit list instead, one shard per entry
    (a device may repeat: concurrent shards on one GPU); decode() then splits a
    batch in len(devices) contiguous slices, one host thread each.
    host_only: plan without touching a device (inspection; cannot decode).
    layout: "auto" (the planner's choice) or "frame_per_lane" — 64 frames per
    wave and a launch sequence per iteration, no waiting between workgroups
    (qldpc_graph_create_opts; canonical adjacency only)."""

    def __init__(self, H: HMatrix, device_mask: int = 0, devices=None, host_only: bool = False,
                 layout: str = "auto"):
        self.H = H
        self.n, self.m = H.n, H.m
        g = ctypes.c_void_p()
        self.host_only = bool(host_only)
        if layout not in _lib.LAYOUTS:
            raise ValueError(f"layout must be one of {sorted(_lib.LAYOUTS)}")
        self.layout = layout
        if layout != "auto":
            opts = _lib.qldpc_graph_opts(_lib.LAYOUTS[layout], 1 if host_only else 0)
            if devices is None and device_mask:
                devices = [d for d in range(31) if device_mask >> d & 1]
            dl = None if devices is None else np.ascontiguousarray(devices, np.int32)
            check(lib().qldpc_graph_create_opts(H.n, H.m, ptr(H.row_ptr), ptr(H.col_idx), ptr(H.col_ptr),
                                                ptr(H.row_idx), ptr(dl), 0 if dl is None else int(dl.size),
                                                ctypes.byref(opts), ctypes.byref(g)), "qldpc_graph_create_opts")
        elif host_only and not _canonical_adjacency(H):
            # (the host-only planner takes check_nodes only and assumes bit_nodes
            # is their ascending transpose; the reference's occurrence pairing of
            # other lists needs qldpc_graph_create_checked)
            raise ValueError("unsorted adjacency: use Graph(H) / Graph(H, devices=...)")
        if layout != "auto":
            pass
        elif host_only:
            check(lib().qldpc_graph_create_host(H.n, H.m, ptr(H.row_ptr), ptr(H.col_idx), ctypes.byref(g)),
                  "qldpc_graph_create_host")
        elif devices is not None:
            dl = np.ascontiguousarray(devices, np.int32)
            check(lib().qldpc_graph_create_checked_on(H.n, H.m, ptr(H.row_ptr), ptr(H.col_idx), ptr(H.col_ptr),
                                                      ptr(H.row_idx), ptr(dl), int(dl.size), ctypes.byref(g)),
                  "qldpc_graph_create_checked_on")
        else:
            check(lib().qldpc_graph_create_checked(H.n, H.m, ptr(H.row_ptr), ptr(H.col_idx), ptr(H.col_ptr),
                                                   ptr(H.row_idx), int(device_mask), ctypes.byref(g)),
                  "qldpc_graph_create_checked")
        self._g = g

    def labels(self) -> tuple[np.ndarray, dict]:
        """The decoder's bank-aware label of each bit id, and the relabelling stats."""
        lab = np.empty(self.n, np.int32)
        st = np.zeros(4, np.int64)
        check(lib().qldpc_graph_labels(self._g, ptr(lab), ptr(st)), "qldpc_graph_labels")
        return lab, {"excess_before": int(st[0]), "excess_after": int(st[1]), "cycles_before": int(st[2]),
                     "cycles_after": int(st[3])}

    @property
    def handle(self) -> ctypes.c_void_p:
        return self._g

    def close(self) -> None:
        if getattr(self, "_g", None) is not None and self._g.value:
            lib().qldpc_graph_destroy(self._g)
            self._g = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self) -> dict:
        n, m, nnz, nd = (ctypes.c_int32() for _ in range(4))
        check(lib().qldpc_graph_info(self._g, ctypes.byref(n), ctypes.byref(m), ctypes.byref(nnz), ctypes.byref(nd)),
              "qldpc_graph_info")
        return {"n": n.value, "m": m.value, "nnz": nnz.value, "devices": nd.value}

    def plan(self, device: int = 0, algorithm: int = 0) -> dict:
        """Launch geometry; a host-only graph has no device, so workgroups is None."""
        lanes, epl, wgs, lds = (ctypes.c_int32() for _ in range(4))
        var = ctypes.c_char_p()
        check(lib().qldpc_graph_plan(self._g, device, algorithm, ctypes.byref(lanes), ctypes.byref(epl),
                                     None if self.host_only else ctypes.byref(wgs), ctypes.byref(lds),
                                     ctypes.byref(var)), "qldpc_graph_plan")
        return {"lanes": lanes.value, "edges_per_lane": epl.value,
                "workgroups": None if self.host_only else wgs.value,
                "lds_bytes": lds.value, "variant": var.value.decode()}

    def split_plan(self) -> dict:
        """Split-frame shape (qldpc_graph_split_plan): parts per frame, lanes per
        part, scratch message slots per lane (parts == 1: one workgroup per frame)."""
        k, pl, rg = (ctypes.c_int32() for _ in range(3))
        check(lib().qldpc_graph_split_plan(self._g, ctypes.byref(k), ctypes.byref(pl), ctypes.byref(rg)),
              "qldpc_graph_split_plan")
        return {"parts": k.value, "part_lanes": pl.value, "scratch_slots": rg.value}

    def set_kernel_timing(self, enabled: bool = True) -> None:
        """Bracket every decode kernel launch with HIP events (qldpc_set_kernel_timing)."""
        check(lib().qldpc_set_kernel_timing(self._g, 1 if enabled else 0), "qldpc_set_kernel_timing")

    def last_decode_kernel_ms(self, stream=None, device: int = 0) -> float:
        """Duration of the last timed decode kernel on (device, stream); waits for it."""
        ms = ctypes.c_float(0.0)
        check(lib().qldpc_last_decode_kernel_ms(self._g, device, _stream_ptr(stream, device), ctypes.byref(ms)),
              "qldpc_last_decode_kernel_ms")
        return float(ms.value)

    def last_claim_order(self, stream=None, device: int = 0, cap: int = 1 << 20):
        """(order, weight) of the last decode on (device, stream): the claim
        order and each frame's weight, or (None, None) for index order."""
        order = np.empty(cap, np.int32)
        weight = np.empty(cap, np.int32)
        cnt = ctypes.c_int32(0)
        check(lib().qldpc_last_claim_order(self._g, device, _stream_ptr(stream, device), order.ctypes.data,
                                           weight.ctypes.data, cap, ctypes.byref(cnt)), "qldpc_last_claim_order")
        if cnt.value == 0:
            return None, None
        return order[:cnt.value].copy(), weight[:cnt.value].copy()

    # ---- host-buffer decode (synchronous, shards over the graph's devices) ----
    def _host_frames(self, llr, syndrome):
        llr = np.ascontiguousarray(llr, np.float64)
        syn = np.ascontiguousarray(syndrome, np.uint8)
        if llr.ndim == 1:
            llr = llr[None, :]
        if syn.ndim == 1:
            syn = syn[None, :]
        batch = llr.shape[0]
        if llr.shape != (batch, self.n) or syn.shape != (batch, self.m):
            raise ValueError(f"expected llr ({batch},{self.n}) and syndrome ({batch},{self.m})")
        return llr, syn, batch

    def decode(self, params: Params, llr: np.ndarray, syndrome: np.ndarray, posterior: bool = False) -> DecodeOutput:
        llr, syn, batch = self._host_frames(llr, syndrome)
        bits = np.empty((batch, self.n), np.uint8)
        iters = np.empty(batch, np.uint32)
        ok = np.empty(batch, np.uint8)
        post = np.empty((batch, self.n), np.float64) if posterior else None
        p = params.c()
        check(lib().qldpc_decode_batch(self._g, ctypes.byref(p), batch, ptr(llr), ptr(syn), ptr(bits), ptr(iters),
                                       ptr(ok), ptr(post)), "qldpc_decode_batch")
        return DecodeOutput(bits, iters, ok, post)

    def decode_trace(self, params: Params, llr: np.ndarray, syndrome: np.ndarray, posterior: bool = False,
                     trace_posterior: bool = False) -> TraceOutput:
        """decode() with the per-iteration trace (frame-per-lane graphs only):
        the unsatisfied-check counts, and the posteriors after every bit pass
        when trace_posterior (batch * max_iterations * n doubles)."""
        llr, syn, batch = self._host_frames(llr, syndrome)
        max_it = max(int(params.max_iterations), 0)
        bits = np.empty((batch, self.n), np.uint8)
        iters = np.empty(batch, np.uint32)
        ok = np.empty(batch, np.uint8)
        post = np.empty((batch, self.n), np.float64) if posterior else None
        unsat = np.empty((batch, max_it), np.uint32)
        tpost = np.empty((batch, max_it, self.n), np.float64) if trace_posterior else None
        p = params.c()
        check(lib().qldpc_decode_trace_batch(self._g, ctypes.byref(p), batch, ptr(llr), ptr(syn), ptr(bits),
                                             ptr(iters), ptr(ok), ptr(post), ptr(unsat), ptr(tpost)),
              "qldpc_decode_trace_batch")
        return TraceOutput(bits, iters, ok, post, unsat, tpost)

    # ---- two parties, host buffers (synchronous, shard like decode) ----
    def _host_keys(self, keys, plan):
        """A party's key bytes as [batch, n] rows.  With a plan a row's first
        n_key = n - punctured - shortened entries are the key; rows of exactly
        n_key entries are accepted and padded."""
        k = np.ascontiguousarray(keys, np.uint8)
        if k.ndim == 1:
            k = k[None, :]
        if plan is not None and k.ndim == 2 and k.shape[1] == plan.n_key != self.n:
            k = np.concatenate([k, np.zeros((k.shape[0], self.n - plan.n_key), np.uint8)], axis=1)
        if k.ndim != 2 or k.shape[1] != self.n:
            raise ValueError(f"expected keys (batch,{self.n})" + (f" or (batch,{plan.n_key})" if plan is not None else ""))
        return k, k.shape[0]

    def syndrome(self, keys: np.ndarray, plan: "RatePlan | None" = None, punct_fill: np.ndarray | None = None):
        """Alice's side (qldpc_syndrome_batch): the syndromes of her keys, uint8
        [batch, m].  With a plan: (extended keys uint8 [batch, n], syndromes of
        the extended keys); punct_fill uint8 [batch, n_punct] is her private
        randomness at the punctured positions."""
        k, batch = self._host_keys(keys, plan)
        npun = 0 if plan is None else int(plan.punctured.size)
        fill = None
        if npun:
            if punct_fill is None:
                raise ValueError(f"the plan punctures {npun} positions: pass punct_fill (batch,{npun})")
            fill = np.ascontiguousarray(punct_fill, np.uint8).reshape(-1, npun)
            if fill.shape[0] != batch:
                raise ValueError(f"expected punct_fill ({batch},{npun})")
        syn = np.empty((batch, self.m), np.uint8)
        ext = np.empty((batch, self.n), np.uint8) if plan is not None else None
        check(lib().qldpc_syndrome_batch(self._g, None if plan is None else plan.handle, batch, ptr(k), ptr(fill),
                                         ptr(ext), ptr(syn)), "qldpc_syndrome_batch")
        return syn if plan is None else (ext, syn)

    def reconcile(self, params: Params, keys: np.ndarray, log_p, syndrome: np.ndarray,
                  plan: "RatePlan | None" = None, posterior: bool = False) -> DecodeOutput:
        """Bob's side (qldpc_reconcile_batch): decode from his own keys, log_p
        (one value, or one per frame) and the received syndromes.  With a plan,
        bits are the extended frames: extract_key maps them back to key bits."""
        k, batch = self._host_keys(keys, plan)
        syn = np.ascontiguousarray(syndrome, np.uint8)
        if syn.ndim == 1:
            syn = syn[None, :]
        if syn.shape != (batch, self.m):
            raise ValueError(f"expected syndrome ({batch},{self.m})")
        lp = np.ascontiguousarray(np.broadcast_to(np.asarray(log_p, np.float64), (batch,)))
        bits = np.empty((batch, self.n), np.uint8)
        iters = np.empty(batch, np.uint32)
        ok = np.empty(batch, np.uint8)
        post = np.empty((batch, self.n), np.float64) if posterior else None
        p = params.c()
        check(lib().qldpc_reconcile_batch(self._g, None if plan is None else plan.handle, ctypes.byref(p), batch,
                                          ptr(k), ptr(lp), ptr(syn), ptr(bits), ptr(iters), ptr(ok), ptr(post)),
              "qldpc_reconcile_batch")
        return DecodeOutput(bits, iters, ok, post)

    # ---- two parties, device pointers ----
    def syndrome_device(self, key, syndrome, plan: "RatePlan | None" = None, punct_fill=None, key_ext=None,
                        stream=None, device: int | None = None) -> None:
        """Alice: syndrome [batch, m] of key [batch, n] (with a plan: of the
        extended key, written to key_ext [batch, n] when given)."""
        dev = key.device.index if device is None else device
        check(lib().qldpc_syndrome_batch_device(
            self._g, None if plan is None else plan.handle, dev, int(key.shape[0]), _dp(key), _dp(punct_fill),
            _dp(key_ext), _dp(syndrome), _stream_ptr(stream, dev)), "qldpc_syndrome_batch_device")

    def reconcile_device(self, params: Params, key, log_p, syndrome, bits, iters, ok, plan: "RatePlan | None" = None,
                         llr_ws=None, posterior=None, stream=None, device: int | None = None) -> None:
        """Bob: frames from key [batch, n] and log_p [batch], decoded against the
        received syndrome [batch, m] (read only)."""
        dev = key.device.index if device is None else device
        p = params.c()
        check(lib().qldpc_reconcile_batch_device(
            self._g, None if plan is None else plan.handle, dev, ctypes.byref(p), int(key.shape[0]), _dp(key),
            _dp(log_p), _dp(syndrome), _dp(llr_ws), _dp(bits), _dp(iters), _dp(ok), _dp(posterior),
            _stream_ptr(stream, dev)), "qldpc_reconcile_batch_device")

    def extract_key_device(self, plan: "RatePlan", bits, key_out, stream=None, device: int | None = None) -> None:
        """key_out [batch, n_key] = bits [batch, n] at the plan's key positions."""
        dev = bits.device.index if device is None else device
        check(lib().qldpc_extract_key_device(self._g, None if plan is None else plan.handle, dev, int(bits.shape[0]),
                                             _dp(bits), _dp(key_out), _stream_ptr(stream, dev)),
              "qldpc_extract_key_device")

    # ---- error estimation at the reconciliation stage ----
    def estimate_classes(self, plan: "RatePlan | None" = None):
        """(degree, rows), int32 each: the distinct effective degrees of the
        informative check rows, ascending, and their row counts
        (qldpc_estimate_classes; host only).  Empty: nothing can be estimated."""
        ph = None if plan is None else plan.handle
        cnt = ctypes.c_int32(0)
        check(lib().qldpc_estimate_classes(self._g, ph, 0, ctypes.byref(cnt), None, None), "qldpc_estimate_classes")
        deg, rows = np.empty(cnt.value, np.int32), np.empty(cnt.value, np.int32)
        check(lib().qldpc_estimate_classes(self._g, ph, cnt.value, ctypes.byref(cnt), ptr(deg), ptr(rows)),
              "qldpc_estimate_classes")
        return deg, rows

    def qber_from_weight(self, weight, plan: "RatePlan | None" = None, q_min: float = 1e-4, q_max: float = 0.25,
                         frames_per_weight: int = 1):
        """(qber, log_p), float64 each, from syndrome weights (qldpc_qber_from_weight;
        host only).  frames_per_weight = F: each weight is a sum over F frames."""
        w = np.ascontiguousarray(weight, np.int64).reshape(-1)
        q, lp = np.empty(w.size, np.float64), np.empty(w.size, np.float64)
        check(lib().qldpc_qber_from_weight(self._g, None if plan is None else plan.handle, int(w.size), ptr(w),
                                           int(frames_per_weight), float(q_min), float(q_max), ptr(q), ptr(lp)),
              "qldpc_qber_from_weight")
        return q, lp

    def estimate_qber(self, keys: np.ndarray, syndrome: np.ndarray, plan: "RatePlan | None" = None,
                      q_min: float = 1e-4, q_max: float = 0.25):
        """Bob, before the decode (qldpc_estimate_qber_batch): (qber float64,
        log_p float64, weight int32), [batch] each, from his keys and the
        received syndromes."""
        k, batch = self._host_keys(keys, plan)
        syn = np.ascontiguousarray(syndrome, np.uint8)
        if syn.ndim == 1:
            syn = syn[None, :]
        if syn.shape != (batch, self.m):
            raise ValueError(f"expected syndrome ({batch},{self.m})")
        w = np.empty(batch, np.int32)
        q, lp = np.empty(batch, np.float64), np.empty(batch, np.float64)
        check(lib().qldpc_estimate_qber_batch(self._g, None if plan is None else plan.handle, batch, ptr(k), ptr(syn),
                                              float(q_min), float(q_max), ptr(w), ptr(q), ptr(lp)),
              "qldpc_estimate_qber_batch")
        return q, lp, w

    def corrected_errors(self, keys: np.ndarray, bits: np.ndarray, plan: "RatePlan | None" = None) -> np.ndarray:
        """Bob, after the decode (qldpc_corrected_errors_batch): int32 [batch],
        the key positions at which his key differs from the decoded frame."""
        k, batch = self._host_keys(keys, plan)
        b = np.ascontiguousarray(bits, np.uint8)
        if b.ndim == 1:
            b = b[None, :]
        if b.shape != (batch, self.n):
            raise ValueError(f"expected bits ({batch},{self.n})")
        err = np.empty(batch, np.int32)
        check(lib().qldpc_corrected_errors_batch(self._g, None if plan is None else plan.handle, batch, ptr(k), ptr(b),
                                                 ptr(err)), "qldpc_corrected_errors_batch")
        return err

    def estimate_qber_device(self, key, syndrome, weight=None, qber=None, log_p=None, plan: "RatePlan | None" = None,
                             q_min: float = 1e-4, q_max: float = 0.25, stream=None, device: int | None = None) -> None:
        """Bob: weight int32, qber float64 and log_p float64 [batch] (each
        optional, not all three missing) from key [batch, n] and the received
        syndrome [batch, m].  log_p can go to reconcile_device on the same stream."""
        dev = key.device.index if device is None else device
        check(lib().qldpc_estimate_qber_device(
            self._g, None if plan is None else plan.handle, dev, int(key.shape[0]), _dp(key), _dp(syndrome),
            float(q_min), float(q_max), _dp(weight), _dp(qber), _dp(log_p), _stream_ptr(stream, dev)),
            "qldpc_estimate_qber_device")

    def corrected_errors_device(self, key, bits, errors, plan: "RatePlan | None" = None, stream=None,
                                device: int | None = None) -> None:
        """errors int32 [batch] = the key positions at which key [batch, n]
        differs from the decoded frames bits [batch, n]."""
        dev = key.device.index if device is None else device
        check(lib().qldpc_corrected_errors_device(self._g, None if plan is None else plan.handle, dev,
                                                  int(key.shape[0]), _dp(key), _dp(bits), _dp(errors),
                                                  _stream_ptr(stream, dev)), "qldpc_corrected_errors_device")

    # ---- blind reconciliation: disclosure rounds for the frames that failed ----
    @staticmethod
    def _round_lists(plan, batch, frames, disc):
        if plan is None:
            raise ValueError("a disclosure round needs a rate plan")
        fr = np.ascontiguousarray(frames, np.int32).reshape(-1)
        dc = np.ascontiguousarray([] if disc is None else disc, np.int32).reshape(-1)
        if fr.size > batch:
            raise ValueError(f"{fr.size} listed frames of a batch of {batch}")
        return fr, dc

    def disclose(self, plan: "RatePlan", frames, punct_fill: np.ndarray, disc) -> np.ndarray:
        """Alice's side of a round (qldpc_disclose_batch): her fill at the
        punctured indices disc, for the listed frames: uint8 [n_list, n_disc]."""
        npun = 0 if plan is None else int(plan.punctured.size)
        fill = np.ascontiguousarray(punct_fill, np.uint8).reshape(-1, max(npun, 1))
        fr, dc = self._round_lists(plan, fill.shape[0], frames, disc)
        vals = np.empty((fr.size, dc.size), np.uint8)
        check(lib().qldpc_disclose_batch(self._g, plan.handle, fill.shape[0], fr.size, ptr(fr), ptr(fill), dc.size,
                                         ptr(dc), ptr(vals)), "qldpc_disclose_batch")
        return vals

    def reconcile_round(self, params: Params, keys: np.ndarray, log_p, syndrome: np.ndarray, plan: "RatePlan", frames,
                        disc, vals, out: DecodeOutput | None = None, posterior: bool = False) -> DecodeOutput:
        """Bob's side of a round (qldpc_reconcile_round_batch): the listed frames
        decoded again with the punctured indices disc pinned at vals [n_list,
        n_disc].  Rows `frames` of `out` (the previous round's output; zeros
        when not given) receive this round's results, the others are kept."""
        k, batch = self._host_keys(keys, plan)
        syn = np.ascontiguousarray(syndrome, np.uint8)
        if syn.ndim == 1:
            syn = syn[None, :]
        if syn.shape != (batch, self.m):
            raise ValueError(f"expected syndrome ({batch},{self.m})")
        fr, dc = self._round_lists(plan, batch, frames, disc)
        v = np.ascontiguousarray(np.empty((fr.size, 0)) if vals is None else vals, np.uint8)
        if v.size != fr.size * dc.size or (v.ndim == 2 and v.shape != (fr.size, dc.size)):
            raise ValueError(f"expected vals ({fr.size},{dc.size})")
        v = v.reshape(fr.size, dc.size)
        lp = np.ascontiguousarray(np.broadcast_to(np.asarray(log_p, np.float64), (batch,)))
        if out is None:
            out = DecodeOutput(np.zeros((batch, self.n), np.uint8), np.zeros(batch, np.uint32), np.zeros(batch, np.uint8),
                               np.zeros((batch, self.n), np.float64) if posterior else None)
        want_post = out.posterior is not None
        shapes = (out.bits.shape == (batch, self.n) and out.iterations.shape == (batch,) and
                  out.synd_ok.shape == (batch,) and (not want_post or out.posterior.shape == (batch, self.n)))
        dtypes = (out.bits.dtype == np.uint8 and out.iterations.dtype == np.uint32 and out.synd_ok.dtype == np.uint8 and
                  (not want_post or out.posterior.dtype == np.float64))
        if not (shapes and dtypes):
            raise ValueError(f"out must be a DecodeOutput of {batch} frames")
        p = params.c()
        check(lib().qldpc_reconcile_round_batch(
            self._g, plan.handle, ctypes.byref(p), batch, ptr(k), ptr(lp), ptr(syn), fr.size, ptr(fr), dc.size,
            ptr(dc), ptr(v), ptr(out.bits), ptr(out.iterations), ptr(out.synd_ok),
            ptr(out.posterior) if want_post else None), "qldpc_reconcile_round_batch")
        return out

    def failed_frames_device(self, ok, list_out, count_out, stream=None) -> None:
        """list_out[:count] = the frames with ok == 0, ascending; count_out[0] =
        their count (ok uint8 [batch], list_out int32 [batch], count_out int32 [1])."""
        dev = ok.device.index
        check(lib().qldpc_failed_frames_device(int(ok.shape[0]), _dp(ok), _dp(list_out), _dp(count_out),
                                               _stream_ptr(stream, dev)), "qldpc_failed_frames_device")

    def disclose_device(self, plan: "RatePlan", frames, punct_fill, disc, vals_out, n_list: int | None = None,
                        stream=None, device: int | None = None) -> None:
        """Alice: vals_out [n_list, n_disc] = punct_fill[frames][:, disc] (int32
        device lists; n_list: the entries of `frames` in use, all by default)."""
        dev = punct_fill.device.index if device is None else device
        check(lib().qldpc_disclose_device(
            self._g, None if plan is None else plan.handle, dev, int(frames.shape[0]) if n_list is None else int(n_list),
            _dp(frames), _dp(punct_fill), 0 if disc is None else int(disc.shape[0]), _dp(disc), _dp(vals_out),
            _stream_ptr(stream, dev)), "qldpc_disclose_device")

    def reconcile_round_device(self, params: Params, key, log_p, syndrome, plan: "RatePlan", frames, disc, vals, bits,
                               iters, ok, posterior=None, n_list: int | None = None, stream=None,
                               device: int | None = None) -> None:
        """Bob: the listed frames of key [batch, n] decoded again with the
        punctured indices disc pinned at vals [n_list, n_disc]; rows `frames` of
        bits / iters / ok / posterior ([batch] arrays) receive the results."""
        dev = key.device.index if device is None else device
        p = params.c()
        check(lib().qldpc_reconcile_round_device(
            self._g, None if plan is None else plan.handle, dev, ctypes.byref(p), int(key.shape[0]), _dp(key),
            _dp(log_p), _dp(syndrome), int(frames.shape[0]) if n_list is None else int(n_list), _dp(frames),
            0 if disc is None else int(disc.shape[0]), _dp(disc), _dp(vals), _dp(bits), _dp(iters), _dp(ok),
            _dp(posterior), _stream_ptr(stream, dev)), "qldpc_reconcile_round_device")

    # ---- symmetric blind reconciliation: per-frame positions (a plan is optional) ----
    def _positions(self, positions, writable: bool = False):
        p = positions
        if not (isinstance(p, np.ndarray) and p.dtype == np.int32 and p.ndim == 2 and p.flags.c_contiguous and
                (p.flags.writeable or not writable)):
            raise ValueError("positions must be a C-contiguous int32 array [batch, cap]")
        return p

    def select_positions(self, posterior: np.ndarray, frames, first: int, count: int, positions: np.ndarray,
                         plan: "RatePlan | None" = None) -> np.ndarray:
        """Bob's side of a symmetric round (qldpc_select_positions_batch):
        positions[f, first:first + count] = the `count` candidates of smallest
        |posterior| of each listed frame f, in the order (|posterior| as 63 bits,
        index).  positions is int32 [batch, cap], written in place and returned;
        its columns before `first` are the frame's earlier positions."""
        post = np.ascontiguousarray(posterior, np.float64)
        pos = self._positions(positions, writable=True)
        if post.ndim != 2 or post.shape[1] != self.n or pos.shape[0] != post.shape[0]:
            raise ValueError(f"expected posterior (batch,{self.n}) and positions (batch,cap)")
        fr = np.ascontiguousarray(frames, np.int32).reshape(-1)
        check(lib().qldpc_select_positions_batch(self._g, None if plan is None else plan.handle, post.shape[0], ptr(post),
                                                 fr.size, ptr(fr), int(first), int(count), ptr(pos), pos.shape[1]),
              "qldpc_select_positions_batch")
        return pos

    def disclose_positions(self, ext: np.ndarray, frames, positions: np.ndarray, first: int, count: int,
                           plan: "RatePlan | None" = None) -> np.ndarray:
        """Alice's side (qldpc_disclose_positions_batch): her bits at
        positions[f, first:first + count] of the listed frames, uint8 [n_list,
        count].  ext: her extended keys with a plan, her keys without, in rows
        of at least n bytes."""
        e = np.ascontiguousarray(ext, np.uint8)
        pos = self._positions(positions)
        if e.ndim != 2 or e.shape[1] < self.n or pos.shape[0] != e.shape[0]:
            raise ValueError(f"expected ext (batch,>={self.n}) and positions (batch,cap)")
        fr = np.ascontiguousarray(frames, np.int32).reshape(-1)
        vals = np.empty((fr.size, int(count)), np.uint8)
        check(lib().qldpc_disclose_positions_batch(self._g, None if plan is None else plan.handle, e.shape[0], fr.size,
                                                   ptr(fr), ptr(e), e.shape[1], ptr(pos), pos.shape[1], int(first),
                                                   int(count), ptr(vals)), "qldpc_disclose_positions_batch")
        return vals

    def reconcile_positions_round(self, params: Params, keys: np.ndarray, log_p, syndrome: np.ndarray, frames,
                                  n_disc: int, positions: np.ndarray, vals, plan: "RatePlan | None" = None,
                                  out: DecodeOutput | None = None, posterior: bool = False) -> DecodeOutput:
        """Bob's side (qldpc_reconcile_positions_round_batch): the listed frames
        decoded again with positions[f, :n_disc] pinned at vals [n_list, n_disc].
        Rows `frames` of `out` receive this round's results, like reconcile_round."""
        k, batch = self._host_keys(keys, plan)
        syn = np.ascontiguousarray(syndrome, np.uint8)
        if syn.ndim == 1:
            syn = syn[None, :]
        if syn.shape != (batch, self.m):
            raise ValueError(f"expected syndrome ({batch},{self.m})")
        pos = self._positions(positions)
        fr = np.ascontiguousarray(frames, np.int32).reshape(-1)
        if pos.shape[0] != batch or fr.size > batch:
            raise ValueError(f"expected positions ({batch},cap) and at most {batch} listed frames")
        nd = int(n_disc)
        v = np.ascontiguousarray(np.empty((fr.size, 0)) if vals is None else vals, np.uint8)
        if v.size != fr.size * nd or (v.ndim == 2 and v.shape != (fr.size, nd)):
            raise ValueError(f"expected vals ({fr.size},{nd})")
        v = v.reshape(fr.size, nd)
        lp = np.ascontiguousarray(np.broadcast_to(np.asarray(log_p, np.float64), (batch,)))
        if out is None:
            out = DecodeOutput(np.zeros((batch, self.n), np.uint8), np.zeros(batch, np.uint32), np.zeros(batch, np.uint8),
                               np.zeros((batch, self.n), np.float64) if posterior else None)
        want_post = out.posterior is not None
        shapes = (out.bits.shape == (batch, self.n) and out.iterations.shape == (batch,) and
                  out.synd_ok.shape == (batch,) and (not want_post or out.posterior.shape == (batch, self.n)))
        dtypes = (out.bits.dtype == np.uint8 and out.iterations.dtype == np.uint32 and out.synd_ok.dtype == np.uint8 and
                  (not want_post or out.posterior.dtype == np.float64))
        if not (shapes and dtypes):
            raise ValueError(f"out must be a DecodeOutput of {batch} frames")
        p = params.c()
        check(lib().qldpc_reconcile_positions_round_batch(
            self._g, None if plan is None else plan.handle, ctypes.byref(p), batch, ptr(k), ptr(lp), ptr(syn), fr.size,
            ptr(fr), nd, ptr(pos), pos.shape[1], ptr(v), ptr(out.bits), ptr(out.iterations), ptr(out.synd_ok),
            ptr(out.posterior) if want_post else None), "qldpc_reconcile_positions_round_batch")
        return out

    def select_positions_device(self, posterior, frames, first: int, count: int, pos, plan: "RatePlan | None" = None,
                                n_list: int | None = None, stream=None, device: int | None = None) -> None:
        """Bob: pos[f, first:first + count] (int32 [batch, cap]) = the listed
        frames' candidates of smallest |posterior| [batch, n], in order."""
        dev = posterior.device.index if device is None else device
        check(lib().qldpc_select_positions_device(
            self._g, None if plan is None else plan.handle, dev, int(posterior.shape[0]), _dp(posterior),
            int(frames.shape[0]) if n_list is None else int(n_list), _dp(frames), int(first), int(count), _dp(pos),
            int(pos.shape[1]), _stream_ptr(stream, dev)), "qldpc_select_positions_device")

    def disclose_positions_device(self, ext, frames, pos, first: int, count: int, vals_out,
                                  plan: "RatePlan | None" = None, n_list: int | None = None, stream=None,
                                  device: int | None = None) -> None:
        """Alice: vals_out [n_list, count] = ext[f, pos[f, first:first + count]] & 1
        for the listed frames (ext: uint8 rows of ext.shape[1] >= n bytes)."""
        dev = ext.device.index if device is None else device
        check(lib().qldpc_disclose_positions_device(
            self._g, None if plan is None else plan.handle, dev, int(frames.shape[0]) if n_list is None else int(n_list),
            _dp(frames), _dp(ext), int(ext.shape[1]), _dp(pos), int(pos.shape[1]), int(first), int(count),
            _dp(vals_out), _stream_ptr(stream, dev)), "qldpc_disclose_positions_device")

    def reconcile_positions_round_device(self, params: Params, key, log_p, syndrome, frames, n_disc: int, pos, vals,
                                         bits, iters, ok, plan: "RatePlan | None" = None, posterior=None,
                                         n_list: int | None = None, stream=None, device: int | None = None) -> None:
        """Bob: the listed frames of key [batch, n] decoded again with the
        positions pos[f, :n_disc] pinned at vals [n_list, n_disc]; rows `frames`
        of bits / iters / ok / posterior receive the results."""
        dev = key.device.index if device is None else device
        p = params.c()
        check(lib().qldpc_reconcile_positions_round_device(
            self._g, None if plan is None else plan.handle, dev, ctypes.byref(p), int(key.shape[0]), _dp(key),
            _dp(log_p), _dp(syndrome), int(frames.shape[0]) if n_list is None else int(n_list), _dp(frames),
            int(n_disc), _dp(pos), 0 if pos is None else int(pos.shape[1]), _dp(vals), _dp(bits), _dp(iters), _dp(ok),
            _dp(posterior), _stream_ptr(stream, dev)), "qldpc_reconcile_positions_round_device")

    # ---- device-pointer entries (torch tensors as plumbing) ----
    def decode_device(self, params: Params, llr, syndrome, bits, iters, ok, posterior=None, stream=None,
                      device: int | None = None) -> None:
        dev = llr.device.index if device is None else device
        p = params.c()
        check(lib().qldpc_decode_batch_device(
            self._g, dev, ctypes.byref(p), int(llr.shape[0]), _dp(llr), _dp(syndrome), _dp(bits),
            _dp(iters), _dp(ok), _dp(posterior),
            _stream_ptr(stream, dev)), "qldpc_decode_batch_device")

    def decode_trace_device(self, params: Params, llr, syndrome, bits, iters, ok, posterior=None, unsat=None,
                            trace_posterior=None, stream=None, device: int | None = None) -> None:
        """decode_device with the trace: unsat int32 / uint32 [batch, max_it],
        trace_posterior float64 [batch, max_it, n] (either may be None)."""
        dev = llr.device.index if device is None else device
        p = params.c()
        check(lib().qldpc_decode_trace_batch_device(
            self._g, dev, ctypes.byref(p), int(llr.shape[0]), _dp(llr), _dp(syndrome), _dp(bits),
            _dp(iters), _dp(ok), _dp(posterior), _dp(unsat), _dp(trace_posterior),
            _stream_ptr(stream, dev)), "qldpc_decode_trace_batch_device")

    def build_frames_device(self, alice, bob, log_p, llr, syndrome, stream=None, device: int | None = None) -> None:
        dev = alice.device.index if device is None else device
        check(lib().qldpc_build_frames_device(self._g, dev, int(alice.shape[0]), _dp(alice), _dp(bob),
                                              _dp(log_p), _dp(llr), _dp(syndrome),
                                              _stream_ptr(stream, dev)), "qldpc_build_frames_device")

    def qkd_ldpc_device(self, params: Params, alice, bob, log_p, llr_ws, synd_ws, bits, iters, ok, keys_match,
                        stream=None, device: int | None = None) -> None:
        """QKD_LDPC's per-trial window for a batch, all on device."""
        dev = alice.device.index if device is None else device
        p = params.c()
        check(lib().qldpc_qkd_ldpc_batch_device(
            self._g, dev, ctypes.byref(p), int(alice.shape[0]), _dp(alice), _dp(bob), _dp(log_p),
            _dp(llr_ws), _dp(synd_ws), _dp(bits), _dp(iters), _dp(ok),
            _dp(keys_match), _stream_ptr(stream, dev)), "qldpc_qkd_ldpc_batch_device")


    # ---- the simulation loop's batch seam (host pointers; shards over the devices) ----
    def run_trials(self, params: Params, qber: float, seeds, seed_add: int = 0, plan: "RatePlan | None" = None):
        """run_trial for every seed (src/simulation.cpp:540-576; seed = seeds[t] +
        seed_add) on device through qldpc_run_trials.  -> TrialsOutput."""
        sd = np.ascontiguousarray(seeds, np.uint64)
        cnt = int(sd.size)
        it = np.empty(cnt, np.uint32)
        ok = np.empty(cnt, np.uint8)
        km = np.empty(cnt, np.uint8)
        rt = np.empty(cnt, np.float64)
        q = ctypes.c_double(0.0)
        p = params.c()
        check(lib().qldpc_run_trials(self._g, None if plan is None else plan.handle, ctypes.byref(p), float(qber),
                                     cnt, sd.ctypes.data, int(seed_add) & 0xFFFFFFFFFFFFFFFF, it.ctypes.data,
                                     ok.ctypes.data, km.ctypes.data, rt.ctypes.data, ctypes.byref(q)),
              "qldpc_run_trials")
        return TrialsOutput(it, ok, km, rt, q.value)

    def submit_trials(self, params: Params, qber: float, seeds, seed_add: int = 0,
                      plan: "RatePlan | None" = None) -> "TrialsJob":
        """run_trials in two halves (qldpc_run_trials_submit / _wait): the trials
        are on the devices when this returns; TrialsJob.wait() -> TrialsOutput.
        Lets a driver put the next combination on the GPUs before it collects
        this one."""
        sd = np.ascontiguousarray(seeds, np.uint64)
        cnt = int(sd.size)
        job = TrialsJob(self, plan, cnt)
        p = params.c()
        h = ctypes.c_void_p()
        check(lib().qldpc_run_trials_submit(self._g, None if plan is None else plan.handle, ctypes.byref(p),
                                            float(qber), cnt, sd.ctypes.data, int(seed_add) & 0xFFFFFFFFFFFFFFFF,
                                            job.it.ctypes.data, job.ok.ctypes.data, job.km.ctypes.data,
                                            job.rt.ctypes.data, ctypes.byref(job.q), ctypes.byref(h)),
              "qldpc_run_trials_submit")
        job.handle = h
        return job

    def rate_plan(self, punctured, shortened) -> "RatePlan":
        return RatePlan(self, punctured, shortened)

    def qkd_ldpc_rate_adapt_device(self, plan: "RatePlan", params: Params, alice, bob, punct_alice, punct_bob, log_p,
                                   alice_ext, llr_ws, synd_ws, bits, iters, ok, keys_match, stream=None,
                                   device: int | None = None) -> None:
        """QKD_LDPC_RATE_ADAPT's per-trial window for a batch, all on device."""
        dev = alice.device.index if device is None else device
        p = params.c()
        check(lib().qldpc_qkd_ldpc_rate_adapt_batch_device(
            self._g, plan.handle, dev, ctypes.byref(p), int(alice.shape[0]), _dp(alice), _dp(bob),
            _dp(punct_alice), _dp(punct_bob), _dp(log_p), _dp(alice_ext), _dp(llr_ws),
            _dp(synd_ws), _dp(bits), _dp(iters), _dp(ok), _dp(keys_match),
            _stream_ptr(stream, dev)), "qldpc_qkd_ldpc_rate_adapt_batch_device")

    def build_frames_rate_adapt_device(self, plan: "RatePlan", alice, bob, punct_alice, punct_bob, log_p, alice_ext,
                                       llr, syndrome, stream=None, device: int | None = None) -> None:
        dev = alice.device.index if device is None else device
        check(lib().qldpc_build_frames_rate_adapt_device(
            self._g, plan.handle, dev, int(alice.shape[0]), _dp(alice), _dp(bob), _dp(punct_alice),
            _dp(punct_bob), _dp(log_p), _dp(alice_ext), _dp(llr), _dp(syndrome),
            _stream_ptr(stream, dev)), "qldpc_build_frames_rate_adapt_device")


class RatePlan:
    """Punctured / shortened positions of one adapted rate, on the graph's devices."""

    def __init__(self, graph: Graph, punctured, shortened):
        self.punctured = np.ascontiguousarray(punctured, np.int32)
        self.shortened = np.ascontiguousarray(shortened, np.int32)
        h = ctypes.c_void_p()
        check(lib().qldpc_rate_plan_create(graph.handle, self.punctured.size, self.punctured.ctypes.data,
                                           self.shortened.size, self.shortened.ctypes.data, ctypes.byref(h)),
              "qldpc_rate_plan_create")
        self.handle = h
        self.n_key = graph.n - int(self.punctured.size) - int(self.shortened.size)  # key bits per frame
        self._graph = graph  # keep the graph alive

    def __del__(self):
        if getattr(self, "handle", None) is not None and self.handle.value:
            lib().qldpc_rate_plan_destroy(self.handle)
            self.handle = None


def keys_match_device(alice, bits, out, stream=None) -> None:
    dev = alice.device.index
    check(lib().qldpc_keys_match_device(int(alice.shape[0]), int(alice.shape[1]), _dp(alice), _dp(bits),
                                        _dp(out), _stream_ptr(stream, dev)), "qldpc_keys_match_device")


def _hash_key_len(row_len: int, key_len, seed_size: int, out_len: int) -> int:
    key_len = row_len if key_len is None else int(key_len)
    if not 1 <= key_len <= row_len:
        raise ValueError(f"key_len must be in [1, {row_len}] (the key rows' length)")
    if out_len < 1:
        raise ValueError("out_len must be >= 1")
    if seed_size < key_len + out_len - 1:
        raise ValueError(f"the seed holds {seed_size} entries; key_len + out_len - 1 = {key_len + out_len - 1} are read")
    return key_len


def toeplitz_hash(keys: np.ndarray, seed: np.ndarray, out_len: int, out_lens=None, key_len: int | None = None):
    """The Toeplitz hash of every key row (qldpc_toeplitz_hash_batch), host arrays:
    out[f, i] = XOR_j seed[i + key_len - 1 - j] & keys[f, j], uint8 [batch, out_len].
    key_len (default: the row length) shorter than the rows hashes each row's
    first key_len bytes.  out_lens (int [batch], each in [0, out_len]): frame f
    keeps its first out_lens[f] outputs, the rest of its row is 0."""
    k = np.ascontiguousarray(keys, np.uint8)
    if k.ndim == 1:
        k = k[None, :]
    s = np.ascontiguousarray(seed, np.uint8).reshape(-1)
    out_len = int(out_len)
    key_len = _hash_key_len(k.shape[1], key_len, s.size, out_len)
    lens = None
    if out_lens is not None:
        lens = np.ascontiguousarray(out_lens, np.int32).reshape(-1)
        if lens.size != k.shape[0]:
            raise ValueError(f"expected {k.shape[0]} out_lens")
    out = np.empty((k.shape[0], out_len), np.uint8)
    check(lib().qldpc_toeplitz_hash_batch(k.shape[0], key_len, k.shape[1], ptr(k), out_len, ptr(s), ptr(lens),
                                          ptr(out)), "qldpc_toeplitz_hash_batch")
    return out


def toeplitz_hash_device(keys, seed, out, out_lens=None, key_len: int | None = None, stream=None) -> None:
    """qldpc_toeplitz_hash_device on device tensors: keys uint8 [batch, row],
    seed uint8 [>= key_len + out_len - 1], out uint8 [batch, out_len], out_lens
    int32 [batch] or None.  Asynchronous on `stream` (default: the current one)."""
    dev = keys.device.index
    key_len = _hash_key_len(int(keys.shape[1]), key_len, int(seed.numel()), int(out.shape[1]))
    if int(out.shape[0]) != int(keys.shape[0]) or (out_lens is not None and int(out_lens.numel()) != int(keys.shape[0])):
        raise ValueError(f"out and out_lens must hold {int(keys.shape[0])} frames")
    if out_lens is not None and str(out_lens.dtype) != "torch.int32":
        raise ValueError("out_lens must be an int32 tensor")
    check(lib().qldpc_toeplitz_hash_device(int(keys.shape[0]), key_len, int(keys.shape[1]), _dp(keys),
                                           int(out.shape[1]), _dp(seed), _dp(out_lens), _dp(out),
                                           _stream_ptr(stream, dev)), "qldpc_toeplitz_hash_device")


def toeplitz_block_workspace(block_len: int, out_len: int) -> int:
    """Bytes of workspace qldpc_toeplitz_hash_block_device needs for a block of
    block_len bits and out_len outputs (block_len + out_len - 1 <= 2^27)."""
    need = int(lib().qldpc_toeplitz_block_workspace(int(block_len), int(out_len)))
    if need < 0:
        check(need, "qldpc_toeplitz_block_workspace")
    return need


def _block_shape(rows: int, row_len: int, key_len, n_frames, seed_size: int, out_len: int):
    """-> (key_len, n_list) of a block hash, after the checks of _hash_key_len on the block's length."""
    key_len = row_len if key_len is None else int(key_len)
    if not 1 <= key_len <= row_len:
        raise ValueError(f"key_len must be in [1, {row_len}] (the key rows' length)")
    n_list = rows if n_frames is None else int(n_frames)
    if out_len < 1:
        raise ValueError("out_len must be >= 1")
    if n_list and seed_size < n_list * key_len + out_len - 1:
        raise ValueError(f"the seed holds {seed_size} entries; n_list * key_len + out_len - 1 = "
                         f"{n_list * key_len + out_len - 1} are read")
    return key_len, n_list


def toeplitz_hash_block(keys: np.ndarray, seed: np.ndarray, out_len: int, frames=None, key_len: int | None = None):
    """The Toeplitz hash of ONE block (qldpc_toeplitz_hash_block), host arrays:
    the rows keys[frames[0]], keys[frames[1]], ... (None: every row, in order),
    each cut to key_len, concatenated to L = len(frames) * key_len bits, and
    out[i] = XOR_j seed[i + L - 1 - j] & block[j], uint8 [out_len].  frames may
    come in any order and repeat a row, up to as many entries as keys has rows.
    An empty list hashes nothing: zeros."""
    k = np.ascontiguousarray(keys, np.uint8)
    if k.ndim == 1:
        k = k[None, :]
    s = np.ascontiguousarray(seed, np.uint8).reshape(-1)
    out_len = int(out_len)
    fr = None
    if frames is not None:
        fr = np.ascontiguousarray(frames, np.int64).reshape(-1)
        if fr.size and (int(fr.min()) < 0 or int(fr.max()) >= k.shape[0]):
            raise ValueError(f"frames must lie in [0, {k.shape[0]})")
        fr = fr.astype(np.int32)
    key_len, n_list = _block_shape(k.shape[0], k.shape[1], key_len, None if fr is None else fr.size, s.size, out_len)
    if n_list > k.shape[0]:
        raise ValueError(f"frames holds {n_list} entries; the host entry takes at most the {k.shape[0]} rows of keys")
    out = np.zeros(out_len, np.uint8)
    check(lib().qldpc_toeplitz_hash_block(k.shape[0], n_list, ptr(fr), key_len, k.shape[1], ptr(k), out_len, ptr(s),
                                          ptr(out)), "qldpc_toeplitz_hash_block")
    return out


def toeplitz_hash_block_device(keys, seed, out, frames=None, key_len: int | None = None, workspace=None,
                               stream=None) -> None:
    """qldpc_toeplitz_hash_block_device on device tensors: keys uint8 [batch, row],
    seed uint8 [>= L + out_len - 1], out uint8 [out_len], frames int32 [n_list] or
    None (every row, in order); L = n_list * key_len.  workspace: a uint8 tensor
    of at least toeplitz_block_workspace(L, out_len) bytes (None: allocated
    here).  Asynchronous on `stream` (default: the current one); a raw stream
    handle (an integer, not a torch stream) needs the caller's workspace: one
    allocated here is freed on return and could not be kept for that stream.
    That frames index rows of keys is the caller's contract."""
    dev = keys.device.index
    if workspace is None and stream is not None and not hasattr(stream, "cuda_stream"):
        raise ValueError("a raw stream handle needs a workspace: pass workspace=, or a torch stream")
    if keys.dim() != 2 or out.dim() != 1:
        raise ValueError("keys must be [batch, row] and out [out_len]")
    if frames is not None and str(frames.dtype) != "torch.int32":
        raise ValueError("frames must be an int32 tensor")
    out_len = int(out.numel())
    key_len, n_list = _block_shape(int(keys.shape[0]), int(keys.shape[1]), key_len,
                                   None if frames is None else int(frames.numel()), int(seed.numel()), out_len)
    if n_list == 0:
        return
    if workspace is None:
        import torch

        workspace = torch.empty(toeplitz_block_workspace(n_list * key_len, out_len), dtype=torch.uint8,
                                device=keys.device)
        if stream is not None:  # (freed on return, while the kernels may still run on `stream`)
            workspace.record_stream(stream)
    elif str(workspace.dtype) != "torch.uint8":
        raise ValueError("workspace must be a uint8 tensor")
    check(lib().qldpc_toeplitz_hash_block_device(n_list, _dp(frames), key_len, int(keys.shape[1]), _dp(keys), out_len,
                                                 _dp(seed), _dp(out), _dp(workspace), int(workspace.numel()),
                                                 _stream_ptr(stream, dev)), "qldpc_toeplitz_hash_block_device")


def trial_seeds(simulation_seed: int, count: int) -> np.ndarray:
    """Per-trial seeds of the simulation loop (src/simulation.cpp:713-719)."""
    out = np.empty(count, np.uint64)
    check(lib().qldpc_trial_seeds(int(simulation_seed) & 0xFFFFFFFFFFFFFFFF, int(count), out.ctypes.data),
          "qldpc_trial_seeds")
    return out


def trials_device(n: int, qber: float, seeds, alice, bob, seed_add: int = 0, stream=None) -> float:
    """run_trial's keys for every seed, on device (src/simulation.cpp:540-551).
    seeds: device uint64 tensor [batch]; alice/bob: device uint8 [batch, n].
    Returns the accurate QBER floor(n*qber)/n."""
    import ctypes

    dev = seeds.device.index
    q = ctypes.c_double(0.0)
    check(lib().qldpc_trials_device(int(n), float(qber), int(seeds.shape[0]), _dp(seeds),
                                    int(seed_add) & 0xFFFFFFFFFFFFFFFF, _dp(alice), _dp(bob),
                                    ctypes.byref(q), _stream_ptr(stream, dev)), "qldpc_trials_device")
    return q.value


def xoshiro_state(seed: int) -> np.ndarray:
    st = np.empty(4, np.uint64)
    check(lib().qldpc_xoshiro_state(int(seed) & 0xFFFFFFFFFFFFFFFF, st.ctypes.data), "qldpc_xoshiro_state")
    return st


def adapt_code_rate(n: int, m: int, qber: float, delta: float, efficiency: float, untainted=None, state=None):
    """adapt_code_rate (src/array_and_matrix_operations.cpp:1131-1223).
    state: np.uint64[4] generator state, advanced in place (chain calls like the
    reference's setup loop).  -> (punctured, shortened, adapted_rate); empty
    lists for the reference's skipped (out-of-range) combinations."""
    import ctypes

    if state is None:
        raise ValueError("pass the generator state (xoshiro_state(seed))")
    unt = None if untainted is None else np.ascontiguousarray(untainted, np.int32)
    p = np.empty(n, np.int32)
    s = np.empty(n, np.int32)
    npn, nsn = ctypes.c_int32(0), ctypes.c_int32(0)
    rate = ctypes.c_double(0.0)
    check(lib().qldpc_adapt_code_rate(n, m, qber, delta, efficiency, 0 if unt is None else 1,
                                      None if unt is None else unt.ctypes.data, 0 if unt is None else unt.size,
                                      state.ctypes.data, p.ctypes.data, ctypes.byref(npn), s.ctypes.data,
                                      ctypes.byref(nsn), ctypes.byref(rate)), "qldpc_adapt_code_rate")
    return p[:npn.value].copy(), s[:nsn.value].copy(), rate.value


def select_punctured_untainted(H: "HMatrix", state) -> np.ndarray:
    """select_punctured_bits_untainted (src/array_and_matrix_operations.cpp:
    1002-1067): the untainted puncturing list in selection order — what the
    reference writes to a missing .untp file (:1076-1123).  state: np.uint64[4]
    generator state (xoshiro_state(seed)), advanced in place."""
    import ctypes

    if state is None:
        raise ValueError("pass the generator state (xoshiro_state(seed))")
    rp, ci = np.ascontiguousarray(H.row_ptr, np.int32), np.ascontiguousarray(H.col_idx, np.int32)
    cp, ri = np.ascontiguousarray(H.col_ptr, np.int32), np.ascontiguousarray(H.row_idx, np.int32)
    out = np.empty(H.n, np.int32)
    cnt = ctypes.c_int32(0)
    check(lib().qldpc_select_punctured_untainted(H.n, H.m, rp.ctypes.data, ci.ctypes.data, cp.ctypes.data,
                                                  ri.ctypes.data, state.ctypes.data, out.ctypes.data,
                                                  ctypes.byref(cnt)), "qldpc_select_punctured_untainted")
    return out[:cnt.value].copy()


def trials_rate_adapt_device(n: int, qber: float, seeds, n_punct: int, alice, bob, punct_alice, punct_bob,
                             seed_add: int = 0, stream=None) -> float:
    """trials_device plus QKD_LDPC_RATE_ADAPT's punctured draws (2 per position)."""
    import ctypes

    dev = seeds.device.index
    q = ctypes.c_double(0.0)
    check(lib().qldpc_trials_rate_adapt_device(int(n), float(qber), int(seeds.shape[0]), _dp(seeds),
                                               int(seed_add) & 0xFFFFFFFFFFFFFFFF, int(n_punct), _dp(alice),
                                               _dp(bob), _dp(punct_alice), _dp(punct_bob),
                                               ctypes.byref(q), _stream_ptr(stream, dev)),
          "qldpc_trials_rate_adapt_device")
    return q.value


def _dp(t):
    """Device pointer of a row-major (C-contiguous) tensor: the C ABI reads
    frames as [frame][bit] rows, so a transposed view would be misread."""
    if t is None:
        return None
    if not t.is_contiguous():
        raise ValueError(f"device buffers must be C-contiguous (row-major); got shape {tuple(t.shape)} "
                         f"strides {t.stride()}")
    return t.data_ptr()


def _stream_ptr(stream, device: int):
    if stream is None:
        import torch

        return torch.cuda.current_stream(device).cuda_stream
    return getattr(stream, "cuda_stream", stream)
