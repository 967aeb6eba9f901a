// capi.hip — the C ABI of libqkdldpc_hip.so (include/qkd_ldpc_hip.h): graphs
// on their devices, and the decode, frame-build and trial-generator entries.
//
// A graph's index tables are planned and built on the host (plan.hip,
// layout.hip) and replicated here on each device of the graph.  Decoding is
// the persistent kernel of decoder.hip; the host-buffer entry shards frames
// over devices (one host thread per device, contiguous slices, no
// collectives) — the multi-GPU analogue of the reference's BS::thread_pool
// over trials (src/simulation.cpp:721,740-746).  The host-only entries are in
// host_algos.cpp, the trial pipeline in run_trials.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "estimate_math.h"
#include "graph.hpp"
#include "loaders.hpp"

using namespace qldpc;

namespace qldpc {

thread_local std::string g_last_error;

int fail(int code, const std::string &msg) {
    g_last_error = msg;
    return code;
}
int hip_fail(hipError_t e, const char *what) {
    return fail(QLDPC_EHIP, std::string(what) + ": " + hipGetErrorString(e));
}

}  // namespace qldpc

namespace {

// The graph's tables on the current device: every entry of QLDPC_GRAPH_TABLES
// whose `when` holds for this graph, in the list's order; the first error ends
// it.  (The others stay NULL: the launches test the pointers.)
int upload_tables(DeviceGraph &dg, const qldpc_graph &g, const GraphTables &t) {
    static_assert(T_ALWAYS == 0 && T_FPL == 1 && T_PAIRED == 2 && T_RELABELLED == 3, "exists[] is indexed by TableWhen");
    const bool exists[T_WHEN_COUNT] = {true, g.variant == VAR_FPL, g.paired, t.relabelled()};
    int rc;
#define QLDPC_X(type, name, when, digested) \
    if (exists[when] && (rc = dg.name.upload(t.name))) return rc;
    QLDPC_GRAPH_TABLES(QLDPC_X)
#undef QLDPC_X
    return QLDPC_OK;
}

// Error estimation: the row table of the graph under a plan's position classes
// (cls == NULL: no plan) and the degree classes of its informative rows.
void est_row_table(const qldpc_graph &g, const uint8_t *cls, EstTable &e) {
    e.row_d.assign(std::max(g.m, 1), 0);
    std::map<int32_t, int32_t> classes;
    for (int j = 0; j < g.m; ++j) {
        int d = g.h_row_deg[j];
        for (int k = 0; cls && k < g.h_row_deg[j]; ++k) {
            const uint8_t c = cls[g.h_ell_col[(size_t)k * g.m + j]];
            if (c == 1) {  // a punctured neighbour: Alice's private fill makes the row uniform
                d = 0;
                break;
            }
            d -= c == 2;
        }
        e.row_d[j] = d;
        if (d > 0) ++classes[d];
    }
    e.degree.clear();
    e.rows.clear();
    e.informative = 0;
    for (auto &c : classes) {
        e.degree.push_back(c.first);
        e.rows.push_back(c.second);
        e.informative += c.second;
    }
}

uint64_t adjacency_hash(const qldpc_graph &g) {  // FNV-1a over n, m, the row degrees and the row-ELL columns
    uint64_t h = 0xcbf29ce484222325ull;
    auto mix = [&h](uint32_t v) {
        for (int b = 0; b < 4; ++b) h = (h ^ ((v >> (8 * b)) & 0xffu)) * 0x100000001b3ull;
    };
    mix((uint32_t)g.n);
    mix((uint32_t)g.m);
    for (int32_t v : g.h_row_deg) mix((uint32_t)v);
    for (int32_t v : g.h_ell_col) mix((uint32_t)v);
    return h;
}

// host_only: plan and relabel without any device (introspection; the graph
// has no devices and cannot decode).
// bit_nodes (col_ptr / row_idx, the reference's H_matrix::bit_nodes in its
// own order): NULL means the ascending transpose of check_nodes.
int build_graph(int32_t n, int32_t m, const int32_t *row_ptr, const int32_t *col_idx, int32_t device_mask,
                qldpc_graph **out, bool host_only = false, const std::vector<int> *device_list = nullptr,
                const int32_t *col_ptr = nullptr, const int32_t *row_idx = nullptr, int layout = QLDPC_LAYOUT_AUTO) {
    if (!out) return fail(QLDPC_EINVAL, "out is NULL");
    *out = nullptr;
    DeviceScope restore;  // (outlives g: a graph dropped on an error selects its devices as it goes)
    std::unique_ptr<qldpc_graph> g;
    GraphTables t;
    if (int rc = build_layout(n, m, row_ptr, col_idx, col_ptr, row_idx, g, t, layout)) return rc;
    g->h_ell_col = t.ell_col;
    g->h_row_deg = t.row_deg;
    g->adjacency = adjacency_hash(*g);
    est_row_table(*g, nullptr, g->est);
    g->est.row_d.clear();  // (it is row_deg: the launches pass that)
    if (host_only) {
        *out = g.release();
        return QLDPC_OK;
    }

    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    std::vector<int> devices;
    if (device_list) {
        for (int d : *device_list)
            if (d < 0 || d >= ndev) return fail(QLDPC_EINVAL, "device list names a device that does not exist");
        devices = *device_list;
    } else if (device_mask == 0) {
        int cur = 0;
        HIP_TRY(hipGetDevice(&cur));
        devices.push_back(cur);
    } else {
        for (int d = 0; d < 31; ++d)
            if (device_mask & (1 << d)) {
                if (d >= ndev) return fail(QLDPC_EINVAL, "device_mask names a device that does not exist");
                devices.push_back(d);
            }
    }
    if (int rc = restore.save()) return rc;
    for (int d : devices) {
        auto dg = std::make_unique<DeviceGraph>();
        dg->device = d;
        HIP_TRY(hipSetDevice(d));
        HIP_TRY(hipDeviceGetAttribute(&dg->num_cus, hipDeviceAttributeMultiprocessorCount, d));
        if (int rc = upload_tables(*dg, *g, t)) return rc;
        g->devs.push_back(std::move(dg));
    }
    *out = g.release();
    return QLDPC_OK;
}

DeviceGraph *find_dev(qldpc_graph *g, int device) {
    for (auto &d : g->devs)
        if (d->device == device) return d.get();
    return nullptr;
}

}  // namespace

int qldpc::check_params(const qldpc_params *p) {
    if (!p) return fail(QLDPC_EINVAL, "params is NULL");
    if (p->algorithm < 0 || p->algorithm > 5) return fail(QLDPC_EINVAL, "algorithm must be 0..5");
    if (p->max_iterations < 1) return fail(QLDPC_EINVAL, "max_iterations must be >= 1");
    if (p->thr_enabled && !(p->thr > 0.)) return fail(QLDPC_EINVAL, "threshold must be > 0 when enabled");
    return QLDPC_OK;
}

namespace {

// Per-workgroup scratch of the V2 kernels: overflow message slots, then the VN stage.
// Hybrid min-sum with rows in global scratch: their offset (16-byte aligned).
long long v2_rows_offset(const qldpc_graph &g) {
    return ((long long)g.v2RG * REG_TSTRIDE + g.stage_doubles + 1) / 2 * 2;
}

// v1: the kernel's scratch, plus (occurrence pairing) a slot-major b2c buffer
long long v1_scratch_doubles(const qldpc_graph &g) {
    return scratch_doubles_for(g.variant, g.n, g.m, g.T, g.EPL) + (g.paired ? (long long)g.EPL * g.T : 0);
}

// Relabelled graphs: a non-paletted frame's llr[] in label order, per workgroup
// (DecodeArgs::llr_lab_wg_offset), after everything else; -1: not relabelled.
long long v2_llr_lab_offset(const qldpc_graph &g) {
    if (g.split_k > 1 || g.col_lab.empty()) return -1;
    const long long end = g.rows_global_ms ? v2_rows_offset(g) + 2LL * g.m
                                           : (long long)g.v2RG * REG_TSTRIDE + g.stage_doubles;
    return (end + 31) / 32 * 32;
}

long long v2_scratch_doubles(const qldpc_graph &g) {
    // split frames: the stage is per frame (Workspace::gstage); only the
    // scratch message slots of a V2_RG_SPLIT plan are per workgroup
    if (g.split_k > 1) return g.v2RG > 0 ? (long long)g.v2RG * REG_TSTRIDE : 32;
    long long end = g.rows_global_ms ? v2_rows_offset(g) + 2LL * g.m
                                     : (long long)g.v2RG * REG_TSTRIDE + g.stage_doubles;
    if (v2_llr_lab_offset(g) >= 0) end = v2_llr_lab_offset(g) + g.n;
    return (end + 31) / 32 * 32;
}

// Per-stream workspace of a device graph, created on first use.
Workspace *workspace(DeviceGraph *dg, hipStream_t stream) { return &dg->ws[(void *)stream]; }

// Workspace growth: buffers whose capacity `cap` is below `need` are
// reallocated by `alloc` once the stream's work on the old ones has ended.  The
// capacity reads 0 while they are invalid (an allocation failed).
template <typename Alloc>
int grow(size_t &cap, size_t need, hipStream_t stream, Alloc alloc) {
    if (need <= cap) return QLDPC_OK;
    HIP_TRY(hipStreamSynchronize(stream));
    cap = 0;
    if (int rc = alloc()) return rc;
    cap = need;
    return QLDPC_OK;
}

// Ensure the workspace holds V2 frame codes for `batch` frames (caller holds dg->mu).
int ensure_codes(qldpc_graph *g, Workspace *w, int batch, hipStream_t stream) {
    const size_t nc = (size_t)(g->n + 3) / 4;
    return grow(w->code_frames, (size_t)batch, stream, [&] {
        int rc;
        if ((rc = w->codes.alloc((size_t)batch * nc)) || (rc = w->palette.alloc((size_t)batch * 4))) return rc;
        return w->pal_ok.alloc((size_t)batch);
    });
}

// The device frame builders stage the frame's keys in LDS as bit words
// (decoder.hpp build_frames_lds / build_frames_ra_lds): refuse larger graphs
// with a message instead of a launch error.  (Plain frames: n <= 655,360;
// rate-adapted: n <= ~436k; the reference's codes stop at n = 102,400.)
int frame_builder_fits(const qldpc_graph *g, int n_punct /* < 0: plain frames */) {
    const size_t lds = n_punct < 0 ? build_frames_lds(g->n) : build_frames_ra_lds(g->n, n_punct);
    if (lds <= LDS_MAX_BYTES) return QLDPC_OK;
    return fail(QLDPC_EUNSUP, "n = " + std::to_string(g->n) + ": the device frame builder keeps the frame's keys in " +
                                  "LDS (" + std::to_string(lds) + " bytes > " + std::to_string(LDS_MAX_BYTES) +
                                  "); decode such frames through qldpc_decode_batch[_device] with host-built LLRs");
}

// Split frames in flight per physical device.  A part group forms from K
// workgroups of ONE launch resident on one XCD (the claim counter is per launch
// and XCD).  Two persistent split launches that are each only partly resident
// could wait on each other's workgroups until the group timeout — but only if
// each holds fewer than K of an XCD's S workgroup slots, which cannot happen
// when two launches fill the XCD and 2 (K - 1) < S: one of them then has >= K
// there, its groups complete, and its workgroups leave when its frames run out.
// So a split launch (hipStreamWaitEvent, on the GPU) always waits for the split
// launch two before it on its device (at most two in flight), and also for
// the previous one unless both have the same shape (K, part size, LDS: the
// same S) with 2 (K - 1) < S and batches of at most 2048 frames
// (every shipped plan: K <= 16 of S = 64 8-wave or 32 16-wave slots).  The
// 2-stream bench and the batch seam then still start batch i + 1's frames in
// batch i's tail.  One-workgroup frames have no such coupling.
//
// Process lifetime: the events are raw handles and never released.  A static
// destructor must not call into the HIP runtime, which may already be gone at
// exit.
struct SplitSerial {
    std::mutex mu;
    hipEvent_t ev[2] = {nullptr, nullptr};  // the last two split launches' ends
    long long shape[2] = {-1, -1};          // K, part lanes and LDS bytes of that launch
    bool overlap_ok[2] = {false, false};    // 2 (K - 1) < S for that launch
    int last = -1;                          // ev[last] is the most recent (-1: none yet)
};
SplitSerial &split_serial(int device) {
    static std::mutex mu;
    static std::map<int, std::unique_ptr<SplitSerial>> per_device;
    std::lock_guard<std::mutex> lk(mu);
    auto &p = per_device[device];
    if (!p) p.reset(new SplitSerial);
    return *p;
}

// One split launch's turn on its device: wait() makes the stream wait for the
// launches it must not overlap, record() marks the end of this one.  The
// device's lock is held from wait() until record() returns (or the turn ends).
class SplitTurn {
    SplitSerial *ser_ = nullptr;
    std::unique_lock<std::mutex> lk_;
    int slot_ = 0;
    bool ok_ = false;
    long long shape_ = -1;

public:
    int wait(int device, const LaunchShape &s, int wgs, int batch, hipStream_t stream) {
        ser_ = &split_serial(device);
        lk_ = std::unique_lock<std::mutex>(ser_->mu);
        for (auto &e : ser_->ev)
            if (!e) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        const int slots_per_xcd = wgs / 8;  // (8 XCDs; every workgroup of the device is launched)
        // (batches of <= 2048 frames: a group that waits for the other launch to
        // leave its XCD waits at most that launch's run — at 50 iterations of a
        // C4 frame ~0.6 s — well inside the group timeout of ~4 s)
        ok_ = 2 * (s.split_k - 1) < slots_per_xcd && batch <= 2048;
        shape_ = ((long long)s.split_k << 48) | ((long long)s.part_lanes << 32) | (long long)s.lds_bytes;
        if (ser_->last >= 0) {
            const int prev = ser_->last, older = prev ^ 1;
            if (ser_->shape[older] >= 0) HIP_TRY(hipStreamWaitEvent(stream, ser_->ev[older], 0));
            if (!(ok_ && ser_->overlap_ok[prev] && ser_->shape[prev] == shape_))
                HIP_TRY(hipStreamWaitEvent(stream, ser_->ev[prev], 0));
        }
        slot_ = ser_->last < 0 ? 0 : ser_->last ^ 1;
        return QLDPC_OK;
    }
    int record(hipStream_t stream) {
        HIP_TRY(hipEventRecord(ser_->ev[slot_], stream));
        ser_->shape[slot_] = shape_;
        ser_->overlap_ok[slot_] = ok_;
        ser_->last = slot_;
        lk_.unlock();
        return QLDPC_OK;
    }
};

}  // namespace

// Split frames: after the stream is idle, fail loudly if a part group timed
// out waiting for its members (the kernel never hangs on it; results are void).
int qldpc::split_check(qldpc_graph *g, DeviceGraph *dg, hipStream_t stream) {
    if (g->variant != VAR_V2 || g->split_k <= 1) return QLDPC_OK;
    int *ctl = nullptr;
    {
        std::lock_guard<std::mutex> lk(dg->mu);  // ws is shared with other streams' calls
        ctl = workspace(dg, stream)->split_ctl.get();
    }
    if (!ctl) return QLDPC_OK;
    int err = 0;
    HIP_TRY(hipMemcpy(&err, ctl + 16, sizeof(int), hipMemcpyDeviceToHost));
    if (err) return fail(QLDPC_EHIP, "split frame: a part group failed to meet (results void)");
    return QLDPC_OK;
}

namespace {

// DecodeArgs::exit_gate of a launch (decoder_v2.hip, the SPA register shapes'
// parity-only pass): V2_EXIT_GATE, or QLDPC_EXIT_GATE under the diagnostic
// switch (-1: never run the pass; INT_MAX: before every checked scan).  It
// changes when the pass runs, never a result.
int exit_gate() { return env_int("QLDPC_EXIT_GATE", V2_EXIT_GATE); }

// Frame-per-lane workspace budget per (device, stream): a batch whose tiles
// need more runs as consecutive chunks of tiles on the same stream.  4 GiB
// holds 13-16 tiles (832-1024 frames) of the n = 102,400 codes.
constexpr size_t FPL_BUDGET_BYTES = (size_t)4 << 30;

// The device-resident frames of one decode call (post, frame_clk: nullable).
struct Frames {
    int batch;
    const double *llr;
    const uint8_t *synd;
    uint8_t *bits;
    uint32_t *iters;
    uint8_t *ok;
    double *post;
    uint64_t *frame_clk;
    // the per-iteration trace (qldpc_decode_trace_batch*, frame-per-lane graphs only; nullable)
    uint32_t *trace_unsat;  // [batch][max_iterations]
    double *trace_post;     // [batch][max_iterations][n]
};

// ---- the steps of a decode call (decode_on, decode_fpl_on) ---------------------

// Resident workgroups per CU of a launch on dg's device (the current one), 0
// when its kernel cannot be resident.  Cached per algorithm: no launch-time
// knob moves what occupancy_proxy() asks.  Caller holds dg->mu.
int blocks_per_cu(DeviceGraph *dg, const LaunchShape &s, int *blocks) {
    int &b = dg->occ[s.alg];
    if (b == 0) {
        const hipError_t e = s.variant == VAR_V2 ? occupancy_v2(s.occupancy_proxy(), &b)
                                                 : occupancy(s.variant, s.alg, s.threads, s.lds_bytes, &b);
        if (e != hipSuccess) {
            b = 0;
            return hip_fail(e, "occupancy");
        }
    }
    *blocks = b;
    return QLDPC_OK;
}

constexpr size_t split_ctl_words(size_t slots) { return 32 + 3 * 16 * slots; }

// Workgroups of the launch, and the stream's workspace grown to hold `batch`
// frames of it (a stream sync only when a buffer grows).
int decode_workspace(qldpc_graph *g, DeviceGraph *dg, const LaunchShape &s, int batch, bool codes_ready,
                     hipStream_t stream, Workspace **ws, int *workgroups) {
    const bool v2 = s.variant == VAR_V2, split = s.split_k > 1;
    std::lock_guard<std::mutex> lk(dg->mu);
    int b = 0, rc;
    if ((rc = blocks_per_cu(dg, s, &b))) return rc;
    if (b <= 0) return fail(QLDPC_EUNSUP, "decoder kernel cannot be resident with this graph shape");
    int wgs = std::min(batch, b * dg->num_cus);
    // split frames: every workgroup of the device (each XCD must hold whole
    // part groups; the claim protocol needs >= split_k of them per XCD)
    if (split) {
        wgs = b * dg->num_cus;
        // QLDPC_SPLIT_WGS (A/B): fewer workgroups, so fewer frames share an
        // XCD's L2 (whole XCD rounds of 8; every XCD keeps >= split_k)
        const int lim = env_int("QLDPC_SPLIT_WGS", 0);
        if (lim >= 8 * s.split_k && lim < wgs) wgs = lim - lim % 8;
    }
    Workspace *w = workspace(dg, stream);
    if (!w->counter && (rc = w->counter.alloc(16))) return rc;
    if (v2) {
        if (codes_ready && (size_t)batch > w->code_frames)
            return fail(QLDPC_EINVAL, "frame codes were not built for this batch");
        if ((rc = ensure_codes(g, w, batch, stream))) return rc;
    }
    if (split && (rc = grow(w->split_frames, (size_t)batch, stream, [&] {
            int r;
            if ((r = w->split_ctl.alloc(split_ctl_words((size_t)batch + 64))) ||
                (r = w->gtotal.alloc((size_t)batch * (g->n + 1))))
                return r;
            return w->gstage.alloc((size_t)batch * std::max<long long>(1, g->stage_doubles));
        })))
        return rc;
    const size_t need = (size_t)(v2 ? v2_scratch_doubles(*g) : v1_scratch_doubles(*g)) * (size_t)wgs;
    if ((rc = grow(w->scratch_doubles, need, stream, [&] { return w->scratch.alloc(need); }))) return rc;
    *ws = w;
    *workgroups = wgs;
    return QLDPC_OK;
}

// The frame-per-lane decoder's workspace, grown to `chunk` tiles.
int fpl_workspace(DeviceGraph *dg, size_t chunk, size_t tile_words, hipStream_t stream, Workspace **ws) {
    std::lock_guard<std::mutex> lk(dg->mu);
    Workspace *w = workspace(dg, stream);
    *ws = w;
    return grow(w->fpl_tiles, chunk, stream, [&] { return w->fpl.alloc(chunk * tile_words); });
}

// Claim order: hardest-looking frames first (order.hip), for batches of at
// least min_batch frames; QLDPC_ORDER=0: index order.  It only schedules —
// results never depend on it — so a shape it cannot run (LDS beyond the device
// limit) decodes in index order instead.  *order: the order, or nullptr.
int claim_order(const qldpc_graph *g, DeviceGraph *dg, Workspace *w, const Frames &f, int min_batch,
                hipStream_t stream, const int32_t **order) {
    const size_t batch = (size_t)f.batch;
    {
        std::lock_guard<std::mutex> lk(dg->mu);
        if (int rc = grow(w->order_frames, batch, stream, [&] {
                const int r = w->fweight.alloc(batch);
                return r ? r : w->forder.alloc(batch);
            }))
            return rc;
    }
    *order = nullptr;
    const char *e = qldpc_diag_env("QLDPC_ORDER");
    if (!(e && std::strcmp(e, "0") == 0) && f.batch >= min_batch) {
        // (V2 reads the frame codes; on relabelled graphs they are in label order, so is the row-ELL it reads)
        const bool v2 = g->variant == VAR_V2;
        const hipError_t oe = launch_frame_order(
            g->n, g->m, dg->col_orig ? dg->ell_lab.get() : dg->ell_col.get(), dg->row_deg.get(), f.batch, f.synd, f.llr,
            v2 ? w->codes.get() : nullptr, v2 ? w->palette.get() : nullptr, v2 ? w->pal_ok.get() : nullptr,
            w->fweight.get(), w->forder.get(), dg->col_orig.get(), stream);
        if (oe == hipSuccess) *order = w->forder.get();
        else (void)hipGetLastError();  // clear the sticky launch error; index order
    }
    w->order_count = *order ? f.batch : 0;
    return QLDPC_OK;
}

// Timing bracket (qldpc_set_kernel_timing): events around the decode launches.
// (The workspace is per stream: no other call records on these events.)
int timing_begin(const qldpc_graph *g, Workspace *w, hipStream_t stream) {
    if (!g->kernel_timing) return QLDPC_OK;
    if (!w->ev0) HIP_TRY(hipEventCreate(w->ev0.put()));
    if (!w->ev1) HIP_TRY(hipEventCreate(w->ev1.put()));
    HIP_TRY(hipEventRecord(w->ev0, stream));
    return QLDPC_OK;
}
int timing_end(const qldpc_graph *g, Workspace *w, hipStream_t stream) {
    if (!g->kernel_timing) return QLDPC_OK;
    HIP_TRY(hipEventRecord(w->ev1, stream));
    w->ev_recorded = true;
    return QLDPC_OK;
}

// Diagnostic stamp build (QL_PHASE_STAMPS, never the product): the launch's
// per-wave phase stamps, reported as each phase's share of wave time in one
// JSON line on stderr.  The product's is empty.
struct PhaseStamps {
#ifdef QL_PHASE_STAMPS
    DevBuf<uint64_t> d_st;
    size_t nst = 0;
    int begin(DecodeArgs &a, int wgs, int threads, hipStream_t stream) {
        nst = (size_t)wgs * (threads / 64) * NUM_STAMPS;
        if (int rc = d_st.alloc(nst)) return rc;
        HIP_TRY(hipMemsetAsync(d_st.get(), 0, nst * sizeof(uint64_t), stream));
        a.stamps = d_st.get();
        return QLDPC_OK;
    }
    int report(hipStream_t stream) {
        std::vector<uint64_t> h(nst);
        HIP_TRY(hipStreamSynchronize(stream));
        HIP_TRY(hipMemcpy(h.data(), d_st.get(), nst * sizeof(uint64_t), hipMemcpyDeviceToHost));
        double tot[NUM_STAMPS] = {0}, all = 0;
        for (size_t i = 0; i < nst; ++i) tot[i % NUM_STAMPS] += (double)h[i];
        for (int i = 0; i < NUM_STAMPS; ++i) all += tot[i];
        std::string js = "{\"phase_stamps\": {";
        for (int i = 0; i < NUM_STAMPS; ++i)
            js += std::string(i ? ", " : "") + "\"" + STAMP_NAMES[i] + "\": " + std::to_string(all > 0 ? tot[i] / all : 0.);
        js += "}, \"wave_cycles_total\": " + std::to_string(all) + "}";
        fprintf(stderr, "%s\n", js.c_str());
        return QLDPC_OK;
    }
#else
    int begin(DecodeArgs &, int, int, hipStream_t) { return QLDPC_OK; }
    int report(hipStream_t) { return QLDPC_OK; }
#endif
};

// The SPA clip constants of a threshold setting, for the decode launch and the
// math self-test alike (thr_on false: clipping at +inf).
SpaClip spa_clip(bool thr_on, double thr) {
    SpaClip c;
    c.thr = thr_on ? thr : HUGE_VAL;
    c.lim = c.thr < 44.0 ? c.thr : 44.0;
    c.t_lim = std::tanh(c.lim / 2.);
    c.c_top = 2. * std::atanh(0x1.fffffffffffffp-1);
    return c;
}

// The kernel arguments of a V1 / V2 launch: what the shape chose decides every
// table and offset here (frame_order is the claim-order step's).
DecodeArgs fill_args(const qldpc_graph *g, const DeviceGraph *dg, const Workspace *w, const LaunchShape &s,
                     const qldpc_params *p, const Frames &f) {
    const int alg = s.alg;
    const bool v2 = s.variant == VAR_V2, split = s.split_k > 1;
    const bool minsum = v2 && alg >= 2;  // V2 min-sum: the tables that list a bit's rows by kpos
    DecodeArgs a{};
    a.n = g->n; a.m = g->m; a.E = g->E; a.T = s.threads; a.EPL = g->EPL; a.dv_max = g->dv_max; a.max_dc = g->max_dc;
    a.lane_row0 = dg->lane_row0.get(); a.lane_head = dg->lane_head.get();
    a.lane_nst = dg->lane_nst.get(); a.lane_epl = dg->lane_epl.get();
    a.slot_meta = minsum ? dg->slot_meta_ms.get() : dg->slot_meta.get();
    a.vn_mask = minsum ? dg->vn_mask_ms.get() : dg->vn_mask.get();
    a.vn_exec = minsum ? dg->vn_exec_ms.get() : dg->vn_exec.get();
    a.slot_meta2 = minsum ? dg->slot_meta2_ms.get() : dg->slot_meta2.get();
    a.ell_col = dg->ell_col.get(); a.row_deg = dg->row_deg.get();
    a.alg = alg; a.max_it = p->max_iterations; a.thr_on = p->thr_enabled ? 1 : 0;
    a.thr = p->thr; a.primary = p->primary; a.secondary = p->secondary;
    {
        const bool norm = alg == 2 || alg == 4, adapt = alg == 4 || alg == 5;
        const auto fine = [&](double x) { return norm ? (std::fabs(x) <= 1.0) : (x >= 0.0); };  // NaN: not fine
        a.ms_clip_later = (fine(p->primary) && (!adapt || fine(p->secondary))) ? 0 : 1;
    }
    {
        const SpaClip c = spa_clip(a.thr_on, p->thr);
        a.spa_tlim = c.t_lim;
        a.spa_ctop = c.c_top;
    }
    a.batch = f.batch; a.llr = f.llr; a.synd = f.synd; a.bits = f.bits; a.iters = f.iters; a.ok = f.ok; a.post = f.post;
    a.frame_clk = f.frame_clk;
    a.frame_counter = w->counter.get();
    a.scratch = w->scratch.get();
    a.scratch_wg_doubles = v2 ? v2_scratch_doubles(*g) : v1_scratch_doubles(*g);
    if (!v2 && g->paired) {
        a.pair_src = dg->pair_src.get();
        a.pair_col = dg->pair_col.get();
        a.pair_buf_off = scratch_doubles_for(g->variant, g->n, g->m, g->T, g->EPL);
    }
    a.hd_uniform_dv = g->hd_uniform_dv;
    a.vn_k0 = g->vn_k0; a.n_hd = g->n_hd; a.hd_bits = dg->hd_bits.get(); a.hd_dv = dg->hd_dv.get();
    a.stage_off = dg->stage_off.get();
    a.stage_wg_offset = (long long)g->v2RG * REG_TSTRIDE;
    a.rows_wg_offset = s.rglb ? v2_rows_offset(*g) : -1;
    a.rows_lds = s.rglb ? s.rows_lds : g->m;
    a.rows_lds_waves = s.rglb ? g->rows_lds_waves_ms : (g->T / 64);
    a.wave_rows = dg->wave_rows.get();
    // the rows kept in global scratch fit the totals region below total[n]
    // (dead between the scan and the bit gather): their waves' message pass
    // reads them from an LDS copy (QLDPC_ROWS_COPY=0: from L2, A/B)
    a.rows_copy = (s.rglb && (long long)(g->m - a.rows_lds) * 16 <= (long long)g->n * 8 &&
                   env_int("QLDPC_ROWS_COPY", 1))
                      ? 1 : 0;
    a.row_orig = dg->row_orig.get();
    a.col_orig = dg->col_orig.get();
    a.col_lab = dg->col_lab.get();
    a.llr_lab_wg_offset = (v2 && dg->col_orig) ? v2_llr_lab_offset(*g) : -1;
    a.row_sem = (v2 && g->nst_max > 0) ? dg->row_sem.get() : nullptr;
    a.row_rmask = (v2 && g->nst_max > 0) ? dg->row_rmask.get() : nullptr;
    a.nst_max = g->nst_max;
    a.split_k = s.split_k;
    if (split) {
        const int slots = (int)w->split_frames + 64;
        a.split_mrows = g->split_mrows;
        a.split_slots = slots;
        a.part_row0 = dg->part_row0.get();
        a.split_claim = w->split_ctl.get();
        a.split_err = w->split_ctl.get() + 16;
        a.split_pub = w->split_ctl.get() + 32;
        a.split_sync = a.split_pub + 16 * slots;
        a.split_mis = a.split_sync + 16 * slots;
        a.gtotal = w->gtotal.get();
        a.gstage = w->gstage.get();
        a.stage_frame_doubles = g->stage_doubles;
        a.split_cb = g->split_cb;
        a.split_nc = g->split_nc;
        a.xoff = g->split_cb > 0 ? dg->xoff.get() : nullptr;
        a.xbit = minsum ? dg->xbit_ms.get() : dg->xbit.get();
    }
    a.nc = (g->n + 3) / 4;
    a.codes = w->codes.get(); a.palette = w->palette.get(); a.pal_ok = w->pal_ok.get();
    a.n_iso = g->n_iso; a.iso_bits = dg->iso_bits.get(); a.v2R = g->v2R; a.v2RG = g->v2RG;
    if (s.vng) {  // min-sum bit gather instead of the VN phases
        a.vn_rows = reinterpret_cast<const uint2 *>(dg->vn_rows.get());
        if (s.RG > 0) {
            a.vng_bits = reinterpret_cast<const uint2 *>(dg->vng_bits.get());
            a.slot_meta2 = dg->vng_meta2.get();
        } else {
            a.slot_meta2 = dg->vng_rec.get();
        }
    }
    a.exit_gate = exit_gate();
    return a;
}

// The kernel arguments of a frame-per-lane chunk sequence (tiles / frames / frame0 are each chunk's).
FplArgs fill_fpl_args(const qldpc_graph *g, const DeviceGraph *dg, const Workspace *w, const qldpc_params *p,
                      const Frames &f, size_t chunk) {
    FplArgs a{};
    a.n = g->n; a.m = g->m; a.E = g->E;
    a.row_ptr = dg->fpl_row_ptr.get(); a.col_idx = dg->fpl_col.get();
    a.rows = dg->fpl_rows.get();
    for (int c = 0; c <= FPL_CLASSES; ++c) a.class_off[c] = g->fpl_class_off[c];
    a.cslot = dg->fpl_cslot.get(); a.col_ptr = dg->fpl_col_ptr.get();
    a.alg = p->algorithm; a.max_it = p->max_iterations; a.thr_on = p->thr_enabled ? 1 : 0;
    a.thr = p->thr; a.primary = p->primary; a.secondary = p->secondary;
    a.llr = f.llr; a.synd = f.synd; a.bits = f.bits; a.iters = f.iters; a.ok = f.ok; a.post = f.post;
    a.frame_clk = f.frame_clk;
    // the chunk's arrays, in fpl_tile_words' order
    const size_t c = chunk, n = (size_t)g->n, m = (size_t)std::max(g->m, 1), E = (size_t)g->E;
    uint64_t *at = w->fpl.get();
    a.C = reinterpret_cast<double *>(at); at += c * E * FPL_LANES;
    a.T = reinterpret_cast<double *>(at); at += c * n * FPL_LANES;
    a.L = reinterpret_cast<double *>(at); at += c * n * FPL_LANES;
    a.hard = at; at += c * n;
    a.syn = at; at += c * m;
    a.active = at; at += c;
    a.flags = at;
    return a;
}

// The per-iteration trace exists on the frame-per-lane layout alone.
int trace_layout_check(const qldpc_graph *g) {
    if (g->variant == VAR_FPL) return QLDPC_OK;
    return fail(QLDPC_EUNSUP, "the per-iteration trace needs a graph of the frame-per-lane layout "
                              "(QLDPC_LAYOUT_FRAME_PER_LANE, Graph(H, layout=\"frame_per_lane\"))");
}

// decode_on for a frame-per-lane graph: deal the frames to tiles of 64, then
// enqueue every chunk's launch sequence (decoder_fpl.hip).  Nothing is read
// back: the sequence's length depends on max_iterations and the graph alone.
int decode_fpl_on(qldpc_graph *g, DeviceGraph *dg, const qldpc_params *p, const Frames &f, hipStream_t stream,
                  hipEvent_t before_decode) {
    const size_t tile_words = fpl_tile_words(g->n, g->m, g->E);
    const int tiles_all = (f.batch + FPL_LANES - 1) / FPL_LANES;
    int chunk = (int)std::min<size_t>((size_t)tiles_all, std::max<size_t>(1, FPL_BUDGET_BYTES / (tile_words * 8)));
    {  // QLDPC_FPL_TILES=k (diagnostic switch): k tiles per chunk
        const int k = env_int("QLDPC_FPL_TILES", 0);
        if (k > 0) chunk = std::min(k, tiles_all);
    }
    chunk = std::min(chunk, 65535);  // (tiles are the grids' y dimension)
    Workspace *w;
    int rc;
    if ((rc = fpl_workspace(dg, (size_t)chunk, tile_words, stream, &w))) return rc;
    FplArgs a = fill_fpl_args(g, dg, w, p, f, (size_t)chunk);
    FplTrace trace;
    trace.unsat = f.trace_unsat;
    trace.post = f.trace_post;
    // rows no bit pass writes read QLDPC_TRACE_NONE / an all-ones NaN; the tiles'
    // counters start at zero (the flush step returns them there)
    const size_t trace_rows = (size_t)f.batch * (size_t)p->max_iterations;
    if (trace.unsat) {
        {
            std::lock_guard<std::mutex> lk(dg->mu);
            if ((rc = grow(w->fpl_trace_tiles, (size_t)chunk, stream,
                           [&] { return w->fpl_trace_cnt.alloc((size_t)chunk * FPL_LANES); })))
                return rc;
        }
        trace.cnt = w->fpl_trace_cnt.get();
        HIP_TRY(hipMemsetAsync(trace.cnt, 0, (size_t)chunk * FPL_LANES * sizeof(uint32_t), stream));
        HIP_TRY(hipMemsetAsync(trace.unsat, 0xFF, trace_rows * sizeof(uint32_t), stream));
    }
    if (trace.post) HIP_TRY(hipMemsetAsync(trace.post, 0xFF, trace_rows * (size_t)g->n * sizeof(double), stream));
    // the deal: frames in the claim order's sequence, so that a tile's 64 frames
    // look alike (one tile: index order).  Results are per frame either way.
    if ((rc = claim_order(g, dg, w, f, FPL_LANES + 1, stream, &a.frame_order))) return rc;
    if ((rc = timing_begin(g, w, stream))) return rc;
    if (before_decode) HIP_TRY(hipStreamWaitEvent(stream, before_decode, 0));
    for (int t0 = 0; t0 < tiles_all; t0 += chunk) {
        a.tiles = std::min(chunk, tiles_all - t0);
        a.frame0 = t0 * FPL_LANES;
        a.frames = std::min(f.batch - a.frame0, a.tiles * FPL_LANES);
        HIP_TRY(launch_fpl_chunk(a, trace, stream));
    }
    return timing_end(g, w, stream);
}

// Enqueue the decoder for `batch` device-resident frames on `stream`.  For the
// V2 kernel the frames' palette + codes are taken from the stream's workspace
// when `codes_ready` (written by build_frames), else computed here from llr.
// The decode kernel waits for `before_decode` when given (the kernels that
// prepare it do not).
int decode_on(qldpc_graph *g, DeviceGraph *dg, const qldpc_params *p, int batch, const double *llr,
              const uint8_t *synd, uint8_t *bits, uint32_t *iters, uint8_t *ok, double *post,
              hipStream_t stream, bool codes_ready = false, uint64_t *frame_clk = nullptr,
              hipEvent_t before_decode = nullptr, uint32_t *trace_unsat = nullptr, double *trace_post = nullptr) {
    if (batch == 0) return QLDPC_OK;
    const Frames f{batch, llr, synd, bits, iters, ok, post, frame_clk, trace_unsat, trace_post};
    if (g->variant == VAR_FPL) return decode_fpl_on(g, dg, p, f, stream, before_decode);
    if (trace_unsat || trace_post) return trace_layout_check(g);
    const LaunchShape s = launch_shape(*g, p->algorithm, vng_enabled());  // (per call: the knobs are read at launch)
    if (s.rglb && !s.vng)
        return fail(QLDPC_EUNSUP, "this code's min-sum row aggregates need the bit gather (QLDPC_VNG=0 given)");
    const bool v2 = s.variant == VAR_V2, split = s.split_k > 1;
    Workspace *w;
    int wgs, rc;
    if ((rc = decode_workspace(g, dg, s, batch, codes_ready, stream, &w, &wgs))) return rc;
    DecodeArgs a = fill_args(g, dg, w, s, p, f);
    if (split) HIP_TRY(hipMemsetAsync(w->split_ctl.get(), 0, split_ctl_words(a.split_slots) * sizeof(int), stream));
    if (v2 && !codes_ready)  // (relabelled graphs: the kernel reads a non-paletted frame by label)
        HIP_TRY(launch_palettize(g->n, a.nc, batch, llr, w->codes.get(), w->palette.get(), w->pal_ok.get(),
                                 dg->col_orig.get(), stream));
    if ((rc = claim_order(g, dg, w, f, 2, stream, &a.frame_order))) return rc;
    HIP_TRY(hipMemsetAsync(w->counter.get(), 0, sizeof(int), stream));
    PhaseStamps stamps;
    if ((rc = stamps.begin(a, wgs, s.threads, stream))) return rc;
    SplitTurn turn;  // split launches in flight per device (SplitSerial)
    if (split && (rc = turn.wait(dg->device, s, wgs, batch, stream))) return rc;
    if ((rc = timing_begin(g, w, stream))) return rc;
    if (before_decode) HIP_TRY(hipStreamWaitEvent(stream, before_decode, 0));
    if (v2) HIP_TRY(launch_decode_v2(s, a, wgs, stream));
    else HIP_TRY(launch_decode(s.variant, a, wgs, s.lds_bytes, stream));
    if (split && (rc = turn.record(stream))) return rc;
    if ((rc = timing_end(g, w, stream))) return rc;
    return stamps.report(stream);
}

const qldpc_rate_plan::Dev *plan_dev(const qldpc_rate_plan *plan, int device) {
    const qldpc_rate_plan::Dev *pd = nullptr;
    for (auto &d : plan->devs)
        if (d.device == device) pd = &d;
    return pd;
}

// The host-buffer entries' sharding: contiguous slices of the batch over the
// graph's devices, one host thread per shard, no collectives; the first error
// of any shard is reported.  body(dg, io, f0, nb) runs with the shard's device
// current, its staging stream created and io_mu held: one call at a time per
// device owns the staging buffers and their stream, from the copy-in to the
// completed copy-out, so concurrent host threads on one shared graph (the
// reference's thread pool over trials) serialise there instead of overwriting
// each other's frames.
template <typename Body>
int for_each_shard(qldpc_graph *g, int32_t batch, const char *host_only_msg, Body body) {
    int rc;
    const int G = (int)g->devs.size();
    if (G == 0) return fail(QLDPC_EINVAL, host_only_msg);
    const int per = (batch + G - 1) / G;
    std::vector<int> rcs(G, QLDPC_OK);
    std::vector<std::string> errs(G);
    auto work = [&](int gi) {
        DeviceGraph *dg = g->devs[gi].get();
        const int f0 = gi * per, f1 = std::min(batch, f0 + per), nb = f1 - f0;
        if (nb <= 0) return;
        auto shard = [&]() -> int {
            HIP_TRY(hipSetDevice(dg->device));
            std::lock_guard<std::mutex> io_lk(dg->io_mu);
            HostIO &io = dg->io;
            if (!io.stream) HIP_TRY(hipStreamCreateWithFlags(io.stream.put(), hipStreamNonBlocking));
            return body(dg, io, f0, nb);
        };
        const int r = shard();
        rcs[gi] = r;
        if (r) errs[gi] = g_last_error;
    };
    {
        DeviceScope restore;
        if ((rc = restore.save())) return rc;
        if (G == 1) {
            work(0);
        } else {
            std::vector<std::thread> th;
            for (int gi = 0; gi < G; ++gi) th.emplace_back(work, gi);
            for (auto &t : th) t.join();
        }
    }
    for (int gi = 0; gi < G; ++gi)
        if (rcs[gi]) return fail(rcs[gi], errs[gi]);
    return QLDPC_OK;
}

// The per-party kernels keep a party's key (Alice with a plan: her fill and the
// extended key too) in LDS as bit words (decoder.hpp alice_syndrome_lds /
// bob_frames_lds): refuse larger graphs with a message instead of a launch error.
int party_fits(const qldpc_graph *g, bool alice, int n_punct /* < 0: no plan */) {
    const size_t lds = alice ? alice_syndrome_lds(g->n, n_punct) : bob_frames_lds(g->n);
    if (lds <= LDS_MAX_BYTES) return QLDPC_OK;
    return fail(QLDPC_EUNSUP, "n = " + std::to_string(g->n) + ": the per-party frame kernels keep the key in LDS (" +
                                  std::to_string(lds) + " bytes > " + std::to_string(LDS_MAX_BYTES) +
                                  "); decode such frames through qldpc_decode_batch[_device] with host-built LLRs");
}

// qkd_ldpc_window minus Alice, for `batch` device-resident frames on `s` (the
// current device is dg's): Bob's frames from his key alone, then the decode
// against the syndrome he received.  V2 decoders read the palette codes the
// frame kernel writes into the stream's workspace; the others read llr[] from
// d_llr_ws or, when it is NULL, from the stream workspace's.
int reconcile_window(qldpc_graph *g, DeviceGraph *dg, const qldpc_rate_plan::Dev *pd, const qldpc_params *p, int batch,
                     const uint8_t *d_key, const double *d_log_p, const uint8_t *d_synd, double *d_llr_ws,
                     uint8_t *d_bits_out, uint32_t *d_iters_out, uint8_t *d_synd_ok_out, double *d_post_out,
                     hipStream_t s) {
    const bool v2 = g->variant == VAR_V2;
    uint8_t *codes = nullptr, *pal_ok = nullptr;
    double *palette = nullptr;
    double *llr = d_llr_ws;
    {
        std::lock_guard<std::mutex> lk(dg->mu);
        Workspace *w = workspace(dg, s);
        if (v2) {
            if (int r = ensure_codes(g, w, batch, s)) return r;
            codes = w->codes.get(); palette = w->palette.get(); pal_ok = w->pal_ok.get();
        } else if (!llr) {
            if (int r = grow(w->llr_ws_frames, (size_t)batch, s, [&] { return w->llr_ws.alloc((size_t)batch * g->n); }))
                return r;
            llr = w->llr_ws.get();
        }
    }
    HIP_TRY(launch_bob_frames(g->n, pd ? pd->cls.get() : nullptr, pd ? pd->src.get() : nullptr, batch, d_key, d_log_p,
                              llr, codes, palette, pal_ok, dg->col_orig.get(), s));
    return decode_on(g, dg, p, batch, llr, d_synd, d_bits_out, d_iters_out, d_synd_ok_out, d_post_out, s, v2);
}

// The round's frame kernel keeps Bob's key and one byte per punctured index in
// LDS (decoder.hpp round_frames_lds).
int round_fits(const qldpc_graph *g, int n_punct) {
    const size_t lds = round_frames_lds(g->n, n_punct);
    if (lds <= LDS_MAX_BYTES) return QLDPC_OK;
    return fail(QLDPC_EUNSUP, "n = " + std::to_string(g->n) + ": the disclosure round's frame kernel keeps the key in " +
                                  "LDS (" + std::to_string(lds) + " bytes > " + std::to_string(LDS_MAX_BYTES) +
                                  "); decode such frames through qldpc_decode_batch[_device] with host-built LLRs");
}

// One disclosure round for the frames d_list[0 .. n_list) of `batch` device-
// resident frames on `s` (the current device is dg's): their pinned LLRs and
// syndromes as compact rows in the stream's workspace, the decode of those
// n_list frames from the LLRs (a pinned -DBL_MAX has no palette code), and the
// results scattered to rows d_list[j] of the outputs.  d_list == NULL: the
// frames 0 .. n_list in order (the host entry's staged rows), decoded straight
// into the outputs.  by_position: a symmetric round, which pins the frame's
// own positions d_pos[f][0 .. n_disc) (rows of `cap` entries) instead of the
// punctured indices d_disc, and needs no plan (pd nullable).
int round_window(qldpc_graph *g, DeviceGraph *dg, const qldpc_rate_plan::Dev *pd, int n_punct, const qldpc_params *p,
                 int batch, const uint8_t *d_key, const double *d_log_p, const uint8_t *d_synd, int n_list,
                 const int32_t *d_list, int n_disc, const int32_t *d_disc, const uint8_t *d_vals, uint8_t *d_bits_out,
                 uint32_t *d_iters_out, uint8_t *d_synd_ok_out, double *d_post_out, hipStream_t s,
                 bool by_position = false, const int32_t *d_pos = nullptr, int cap = 0) {
    const size_t n = (size_t)g->n, m = (size_t)g->m, nl = (size_t)n_list;
    double *llr, *cpost = d_post_out;
    uint8_t *synd_ws, *cbits = d_bits_out, *cok = d_synd_ok_out;
    uint32_t *citers = d_iters_out;
    {
        std::lock_guard<std::mutex> lk(dg->mu);
        Workspace *w = workspace(dg, s);
        if (int r = grow(w->round_frames, nl, s, [&] {
                int rc;
                if ((rc = w->round_llr.alloc(nl * n)) || (rc = w->round_synd.alloc(nl * m)) ||
                    (rc = w->round_bits.alloc(nl * n)) || (rc = w->round_ok.alloc(nl)))
                    return rc;
                return w->round_iters.alloc(nl);
            }))
            return r;
        if (d_list && d_post_out)
            if (int r = grow(w->round_post_frames, nl, s, [&] { return w->round_post.alloc(nl * n); })) return r;
        llr = w->round_llr.get();
        synd_ws = w->round_synd.get();
        if (d_list) {
            cbits = w->round_bits.get(); citers = w->round_iters.get(); cok = w->round_ok.get();
            if (d_post_out) cpost = w->round_post.get();
        }
    }
    if (by_position)
        HIP_TRY(launch_positions_frames(g->n, g->m, batch, pd ? pd->cls.get() : nullptr, pd ? pd->src.get() : nullptr,
                                        n_list, d_list, d_key, d_log_p, d_synd, n_disc, d_pos, cap, d_vals, llr,
                                        synd_ws, s));
    else
        HIP_TRY(launch_round_frames(g->n, g->m, batch, n_punct, pd->cls.get(), pd->src.get(), n_list, d_list, d_key,
                                    d_log_p, d_synd, n_disc, d_disc, d_vals, llr, synd_ws, s));
    if (int r = decode_on(g, dg, p, n_list, llr, synd_ws, cbits, citers, cok, cpost, s)) return r;
    if (d_list)
        HIP_TRY(launch_round_scatter(g->n, batch, n_list, d_list, cbits, citers, cok, cpost, d_bits_out, d_iters_out,
                                     d_synd_ok_out, d_post_out, s));
    return QLDPC_OK;
}

}  // namespace

// QKD_LDPC's (plan == NULL) or QKD_LDPC_RATE_ADAPT's per-trial window for
// `batch` device-resident trials on `stream` (the current device is dg's):
// frame build, decode, key comparison.  V2 decoders read the frame builder's
// palette codes, so the f64 LLRs are written only into a caller workspace
// (d_llr_ws, nullable); the other decoders read llr[] from it or, when it is
// NULL, from the stream workspace's.
int qldpc::qkd_ldpc_window(qldpc_graph *g, DeviceGraph *dg, const qldpc_rate_plan *plan, const qldpc_params *p,
                           int batch, const uint8_t *d_alice, const uint8_t *d_bob, const uint8_t *d_punct_alice,
                           const uint8_t *d_punct_bob, const double *d_log_p, uint8_t *d_alice_ext, double *d_llr_ws,
                           uint8_t *d_synd_ws, uint8_t *d_bits_out, uint32_t *d_iters_out, uint8_t *d_synd_ok_out,
                           uint8_t *d_keys_match_out, hipStream_t s, uint64_t *frame_clk, hipEvent_t before_decode) {
    if (batch == 0) return QLDPC_OK;
    const qldpc_rate_plan::Dev *pd = nullptr;
    if (plan) {
        pd = plan_dev(plan, dg->device);
        if (!pd) return fail(QLDPC_EINVAL, "rate plan does not live on that device");
    }
    const bool v2 = g->variant == VAR_V2;
    uint8_t *codes = nullptr, *pal_ok = nullptr;
    double *palette = nullptr;
    double *llr = d_llr_ws;
    {
        std::lock_guard<std::mutex> lk(dg->mu);
        Workspace *w = workspace(dg, s);
        if (v2) {
            // the frame builder writes the V2 palette + codes straight into the
            // stream's workspace, so the decoder skips the palettize pass
            int r = ensure_codes(g, w, batch, s);
            if (r) return r;
            codes = w->codes.get(); palette = w->palette.get(); pal_ok = w->pal_ok.get();
        } else if (!llr) {
            if (int r = grow(w->llr_ws_frames, (size_t)batch, s, [&] { return w->llr_ws.alloc((size_t)batch * g->n); }))
                return r;
            llr = w->llr_ws.get();
        }
    }
    if (int r = frame_builder_fits(g, plan ? plan->n_punct : -1)) return r;
    if (plan)
        HIP_TRY(launch_build_frames_ra(g->n, g->m, dg->ell_col.get(), dg->row_deg.get(), pd->cls.get(), pd->src.get(),
                                       plan->n_punct, batch, d_alice, d_bob, d_punct_alice, d_punct_bob, d_log_p,
                                       d_alice_ext, llr, d_synd_ws, codes, palette, pal_ok, dg->col_orig.get(), s));
    else
        HIP_TRY(launch_build_frames(g->n, g->m, g->max_dc, dg->ell_col.get(), dg->row_deg.get(), batch, d_alice, d_bob,
                                    d_log_p, llr, d_synd_ws, codes, palette, pal_ok, dg->col_orig.get(), s));
    int r = decode_on(g, dg, p, batch, llr, d_synd_ws, d_bits_out, d_iters_out, d_synd_ok_out, nullptr, s, v2,
                      frame_clk, before_decode);
    if (r) return r;
    // keys_match = arrays_equal(alice[_extended], bob_solution) (:1087, :1216)
    if (d_keys_match_out)
        HIP_TRY(launch_keys_match(batch, g->n, plan ? d_alice_ext : d_alice, d_bits_out, d_keys_match_out, s));
    return QLDPC_OK;
}

extern "C" {

const char *qldpc_last_error(void) { return g_last_error.c_str(); }

const char *qldpc_version(void) { return "qkd_ldpc_v_amd 0.1.0 (gfx950)"; }

int32_t qldpc_exit_gate(void) { return exit_gate(); }

int qldpc_device_count(int32_t *count) {
    if (!count) return fail(QLDPC_EINVAL, "count is NULL");
    int c = 0;
    HIP_TRY(hipGetDeviceCount(&c));
    *count = c;
    return QLDPC_OK;
}

int qldpc_load_matrix(const char *path, int32_t format, int32_t *n, int32_t *m, int32_t *nnz, int32_t *row_ptr,
                      int32_t *col_idx, int32_t *col_ptr, int32_t *row_idx, int32_t *is_regular) {
    if (!path || !n || !m || !nnz) return fail(QLDPC_EINVAL, "path/n/m/nnz must not be NULL");
    try {
        const HMatrix H = load_matrix(path, format);
        long long e_rows = 0, e_cols = 0;
        for (const auto &r : H.check_nodes) e_rows += (long long)r.size();
        for (const auto &c : H.bit_nodes) e_cols += (long long)c.size();
        *n = (int32_t)H.bit_nodes.size();
        *m = (int32_t)H.check_nodes.size();
        *nnz = (int32_t)e_rows;
        if (is_regular) *is_regular = H.is_regular ? 1 : 0;
        if (e_rows != e_cols)
            return fail(QLDPC_EINVAL, "check_nodes and bit_nodes hold different edge counts (" +
                                          std::to_string(e_rows) + " vs " + std::to_string(e_cols) + ")");
        if (row_ptr && col_idx) {
            int32_t o = 0;
            for (size_t j = 0; j < H.check_nodes.size(); ++j) {
                row_ptr[j] = o;
                for (int c : H.check_nodes[j]) col_idx[o++] = c;
            }
            row_ptr[H.check_nodes.size()] = o;
        }
        if (col_ptr && row_idx) {
            int32_t o = 0;
            for (size_t i = 0; i < H.bit_nodes.size(); ++i) {
                col_ptr[i] = o;
                for (int r : H.bit_nodes[i]) row_idx[o++] = r;
            }
            col_ptr[H.bit_nodes.size()] = o;
        }
    } catch (const std::exception &e) {
        return fail(QLDPC_EIO, e.what());
    }
    return QLDPC_OK;
}

int qldpc_graph_create(int32_t n, int32_t m, const int32_t *row_ptr, const int32_t *col_idx, int32_t device_mask,
                       qldpc_graph **out) {
    return build_graph(n, m, row_ptr, col_idx, device_mask, out);
}

int qldpc_graph_create_checked(int32_t n, int32_t m, const int32_t *row_ptr, const int32_t *col_idx,
                               const int32_t *col_ptr, const int32_t *row_idx, int32_t device_mask,
                               qldpc_graph **out) {
    if (!row_ptr || !col_idx || !col_ptr || !row_idx) return fail(QLDPC_EINVAL, "NULL adjacency array");
    if (n <= 0 || m < 0) return fail(QLDPC_EINVAL, "invalid graph dimensions");
    // bit_nodes in the caller's order: anything but the ascending transpose of
    // ascending check_nodes rows decodes with the reference's occurrence
    // pairing (layout.hip)
    return build_graph(n, m, row_ptr, col_idx, device_mask, out, false, nullptr, col_ptr, row_idx);
}

int qldpc_graph_create_on(int32_t n, int32_t m, const int32_t *row_ptr, const int32_t *col_idx,
                          const int32_t *devices, int32_t ndevices, qldpc_graph **out) {
    if (!devices || ndevices <= 0 || ndevices > 64) return fail(QLDPC_EINVAL, "need 1..64 devices");
    const std::vector<int> list(devices, devices + ndevices);
    return build_graph(n, m, row_ptr, col_idx, 0, out, false, &list);
}

int qldpc_graph_create_checked_on(int32_t n, int32_t m, const int32_t *row_ptr, const int32_t *col_idx,
                                  const int32_t *col_ptr, const int32_t *row_idx, const int32_t *devices,
                                  int32_t ndevices, qldpc_graph **out) {
    if (!row_ptr || !col_idx || !col_ptr || !row_idx) return fail(QLDPC_EINVAL, "NULL adjacency array");
    if (n <= 0 || m < 0) return fail(QLDPC_EINVAL, "invalid graph dimensions");
    if (!devices || ndevices <= 0 || ndevices > 64) return fail(QLDPC_EINVAL, "need 1..64 devices");
    const std::vector<int> list(devices, devices + ndevices);
    return build_graph(n, m, row_ptr, col_idx, 0, out, false, &list, col_ptr, row_idx);
}

int qldpc_graph_create_host(int32_t n, int32_t m, const int32_t *row_ptr, const int32_t *col_idx,
                            qldpc_graph **out) {
    return build_graph(n, m, row_ptr, col_idx, 0, out, true);
}

int qldpc_graph_create_opts(int32_t n, int32_t m, const int32_t *row_ptr, const int32_t *col_idx,
                            const int32_t *col_ptr, const int32_t *row_idx, const int32_t *devices, int32_t ndevices,
                            const qldpc_graph_opts *opts, qldpc_graph **out) {
    const qldpc_graph_opts none{};
    const qldpc_graph_opts &o = opts ? *opts : none;
    if (o.layout != QLDPC_LAYOUT_AUTO && o.layout != QLDPC_LAYOUT_FRAME_PER_LANE)
        return fail(QLDPC_EINVAL, "unknown layout " + std::to_string(o.layout));
    for (int32_t r : o.reserved)
        if (r) return fail(QLDPC_EINVAL, "qldpc_graph_opts.reserved must be zero");
    if (!row_ptr || !col_idx) return fail(QLDPC_EINVAL, "NULL adjacency array");
    if ((col_ptr == nullptr) != (row_idx == nullptr)) return fail(QLDPC_EINVAL, "col_ptr and row_idx go together");
    if (n <= 0 || m < 0) return fail(QLDPC_EINVAL, "invalid graph dimensions");
    if (o.host_only) return build_graph(n, m, row_ptr, col_idx, 0, out, true, nullptr, col_ptr, row_idx, o.layout);
    if (!devices) return build_graph(n, m, row_ptr, col_idx, 0, out, false, nullptr, col_ptr, row_idx, o.layout);
    if (ndevices <= 0 || ndevices > 64) return fail(QLDPC_EINVAL, "need 1..64 devices");
    const std::vector<int> list(devices, devices + ndevices);
    return build_graph(n, m, row_ptr, col_idx, 0, out, false, &list, col_ptr, row_idx, o.layout);
}

int qldpc_graph_labels(const qldpc_graph *g, int32_t *labels_out, int64_t *stats_out) {
    if (!g) return fail(QLDPC_EINVAL, "graph is NULL");
    if (labels_out)
        for (int i = 0; i < g->n; ++i) labels_out[i] = g->col_lab.empty() ? i : g->col_lab[i];
    if (stats_out)
        for (int i = 0; i < 4; ++i) stats_out[i] = g->relabel_stats[i];
    return QLDPC_OK;
}

void qldpc_graph_destroy(qldpc_graph *g) {
    if (!g) return;
    DeviceScope restore;  // each DeviceGraph selects its device and drains it before its members free
    (void)restore.save();
    delete g;
}

int qldpc_graph_info(const qldpc_graph *g, int32_t *n, int32_t *m, int32_t *nnz, int32_t *num_devices) {
    if (!g) return fail(QLDPC_EINVAL, "graph is NULL");
    if (n) *n = g->n;
    if (m) *m = g->m;
    if (nnz) *nnz = g->E;
    if (num_devices) *num_devices = (int32_t)g->devs.size();
    return QLDPC_OK;
}

int qldpc_graph_plan(const qldpc_graph *g, int32_t device, int32_t algorithm, int32_t *lanes,
                     int32_t *edges_per_lane, int32_t *workgroups, int32_t *lds_bytes, const char **variant) {
    if (!g) return fail(QLDPC_EINVAL, "graph is NULL");
    if (algorithm < 0 || algorithm > 5) return fail(QLDPC_EINVAL, "algorithm must be 0..5");
    DeviceGraph *dg = find_dev(const_cast<qldpc_graph *>(g), device);
    // (a host-only graph answers everything but the device's workgroup count)
    if (!dg && !(g->devs.empty() && !workgroups)) return fail(QLDPC_EINVAL, "graph does not live on that device");
    const LaunchShape s = launch_shape(*g, algorithm, vng_enabled());
    // (split frames: the lanes that run — K parts of split_pl — not the arrays' stride)
    if (lanes) *lanes = s.lanes();
    if (edges_per_lane) *edges_per_lane = g->EPL;
    if (lds_bytes) *lds_bytes = (int32_t)s.lds_bytes;
    if (variant) *variant = s.variant_name();
    if (workgroups && g->variant == VAR_FPL) {
        *workgroups = fpl_cn_grid(g->fpl_class_off);  // the check-node pass's grid for one 64-frame tile
    } else if (workgroups) {
        DeviceScope ds;
        if (int rc = ds.enter(dg->device)) return rc;
        std::lock_guard<std::mutex> lk(dg->mu);
        int b = 0;
        if (int rc = blocks_per_cu(dg, s, &b)) return rc;
        *workgroups = b * dg->num_cus;
    }
    return QLDPC_OK;
}

int qldpc_graph_split_plan(const qldpc_graph *g, int32_t *parts, int32_t *part_lanes, int32_t *scratch_slots) {
    if (!g) return fail(QLDPC_EINVAL, "graph is NULL");
    const bool split = g->variant == VAR_V2 && g->split_k > 1;
    if (parts) *parts = split ? g->split_k : 1;
    if (part_lanes) *part_lanes = split ? g->split_pl : g->T;
    if (scratch_slots) *scratch_slots = g->variant == VAR_V2 ? g->v2RG : 0;
    return QLDPC_OK;
}

int qldpc_set_kernel_timing(qldpc_graph *g, int32_t enabled) {
    if (!g) return fail(QLDPC_EINVAL, "graph is NULL");
    g->kernel_timing = enabled != 0;
    return QLDPC_OK;
}

int qldpc_last_decode_kernel_ms(qldpc_graph *g, int32_t device, void *stream, float *ms) {
    if (!g || !ms) return fail(QLDPC_EINVAL, "graph / ms is NULL");
    DeviceGraph *dg = find_dev(g, device);
    if (!dg) return fail(QLDPC_EINVAL, "graph does not live on that device");
    hipEvent_t e0 = nullptr, e1 = nullptr;
    {
        std::lock_guard<std::mutex> lk(dg->mu);
        auto it = dg->ws.find(stream);
        if (it == dg->ws.end() || !it->second.ev_recorded)
            return fail(QLDPC_EINVAL, "no timed decode launch on that stream (qldpc_set_kernel_timing)");
        e0 = it->second.ev0;
        e1 = it->second.ev1;
    }
    DeviceScope ds;
    if (int rc = ds.enter(device)) return rc;
    hipError_t e = hipEventSynchronize(e1);
    if (e == hipSuccess) e = hipEventElapsedTime(ms, e0, e1);
    if (e != hipSuccess) return hip_fail(e, "decode kernel events");
    return QLDPC_OK;
}

int qldpc_last_claim_order(qldpc_graph *g, int32_t device, void *stream, int32_t *order_out, int32_t *weight_out,
                           int32_t cap, int32_t *count) {
    if (!g || !count) return fail(QLDPC_EINVAL, "graph / count is NULL");
    DeviceGraph *dg = find_dev(g, device);
    if (!dg) return fail(QLDPC_EINVAL, "graph does not live on that device");
    // (the workspace lock is held across the wait and the copies: a decode on
    // the same stream with a larger batch would otherwise free and reallocate
    // forder / fweight under the copy)
    std::lock_guard<std::mutex> lk(dg->mu);
    auto it = dg->ws.find(stream);
    if (it == dg->ws.end()) return fail(QLDPC_EINVAL, "no decode on that stream");
    int32_t *const ord = it->second.forder.get(), *const wt = it->second.fweight.get();
    const int cnt = it->second.order_count;
    *count = cnt;
    if (cnt == 0) return QLDPC_OK;
    if (cap < cnt) return fail(QLDPC_EINVAL, "order buffer smaller than the last batch");
    DeviceScope ds;
    if (int rc = ds.enter(device)) return rc;
    hipError_t e = hipStreamSynchronize(static_cast<hipStream_t>(stream));
    if (e == hipSuccess && order_out) e = hipMemcpy(order_out, ord, (size_t)cnt * sizeof(int32_t), hipMemcpyDeviceToHost);
    if (e == hipSuccess && weight_out) e = hipMemcpy(weight_out, wt, (size_t)cnt * sizeof(int32_t), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_fail(e, "claim order copy");
    return QLDPC_OK;
}

int qldpc_decode_batch_device(qldpc_graph *g, int32_t device, const qldpc_params *p, int32_t batch,
                              const double *d_llr, const uint8_t *d_syndrome, uint8_t *d_bits_out,
                              uint32_t *d_iters_out, uint8_t *d_synd_ok_out, double *d_posterior_out,
                              void *stream) {
    if (!g) return fail(QLDPC_EINVAL, "graph is NULL");
    int rc = check_params(p);
    if (rc) return rc;
    if (batch < 0) return fail(QLDPC_EINVAL, "batch must be >= 0");
    if (batch > 0 && (!d_llr || !d_syndrome || !d_bits_out || !d_iters_out || !d_synd_ok_out))
        return fail(QLDPC_EINVAL, "NULL device buffer");
    DeviceGraph *dg = find_dev(g, device);
    if (!dg) return fail(QLDPC_EINVAL, "graph does not live on that device");
    DeviceScope ds;
    if ((rc = ds.enter(device))) return rc;
    return decode_on(g, dg, p, batch, d_llr, d_syndrome, d_bits_out, d_iters_out, d_synd_ok_out, d_posterior_out,
                     (hipStream_t)stream);
}

// The host-buffer decode behind qldpc_decode_batch and qldpc_decode_trace_batch,
// which have checked the arguments; the trace arrays (nullable) are staged on
// each shard's device for the call.
static int decode_batch_host(qldpc_graph *g, const qldpc_params *p, int32_t batch, const double *llr,
                             const uint8_t *syndrome, uint8_t *bits_out, uint32_t *iters_out, uint8_t *synd_ok_out,
                             double *posterior_out, uint32_t *unsat_out, double *trace_post_out) {
    const size_t n = (size_t)g->n, m = (size_t)g->m;
    return for_each_shard(
        g, batch, "a host-only graph cannot decode", [&](DeviceGraph *dg, HostIO &io, int f0, int nb) -> int {
            if (int r = io.reserve((size_t)nb, n, m, true, true, false)) return r;
            // the shard's trace arrays, for this call alone (allocated before anything is enqueued)
            const size_t rows = (size_t)nb * (size_t)p->max_iterations;
            DevBuf<uint32_t> d_unsat;
            DevBuf<double> d_tpost;
            if ((unsat_out && d_unsat.alloc(rows)) || (trace_post_out && d_tpost.alloc(rows * n))) {
                (void)hipGetLastError();
                return fail(QLDPC_ENOMEM, "no device memory for the trace arrays of " + std::to_string(nb) +
                                              " frames x " + std::to_string(p->max_iterations) + " iterations");
            }
            HIP_TRY(hipMemcpyAsync(io.llr.get(), llr + f0 * n, nb * n * sizeof(double), hipMemcpyHostToDevice, io.stream));
            HIP_TRY(hipMemcpyAsync(io.synd.get(), syndrome + f0 * m, nb * m, hipMemcpyHostToDevice, io.stream));
            int r = decode_on(g, dg, p, nb, io.llr.get(), io.synd.get(), io.bits.get(), io.iters.get(), io.ok.get(),
                              posterior_out ? io.post.get() : nullptr, io.stream, false, nullptr, nullptr,
                              d_unsat.get(), d_tpost.get());
            if (!r && unsat_out) {
                const hipError_t e = hipMemcpyAsync(unsat_out + (size_t)f0 * p->max_iterations, d_unsat.get(),
                                                    rows * sizeof(uint32_t), hipMemcpyDeviceToHost, io.stream);
                if (e != hipSuccess) r = hip_fail(e, "trace copy");
            }
            if (!r && trace_post_out) {
                const hipError_t e = hipMemcpyAsync(trace_post_out + (size_t)f0 * p->max_iterations * n, d_tpost.get(),
                                                    rows * n * sizeof(double), hipMemcpyDeviceToHost, io.stream);
                if (e != hipSuccess) r = hip_fail(e, "trace copy");
            }
            if (r) {
                (void)hipStreamSynchronize(io.stream);  // nothing of this call stays in flight
                return r;
            }
            HIP_TRY(hipMemcpyAsync(bits_out + f0 * n, io.bits.get(), nb * n, hipMemcpyDeviceToHost, io.stream));
            HIP_TRY(hipMemcpyAsync(iters_out + f0, io.iters.get(), nb * sizeof(uint32_t), hipMemcpyDeviceToHost, io.stream));
            HIP_TRY(hipMemcpyAsync(synd_ok_out + f0, io.ok.get(), nb, hipMemcpyDeviceToHost, io.stream));
            if (posterior_out)
                HIP_TRY(hipMemcpyAsync(posterior_out + f0 * n, io.post.get(), nb * n * sizeof(double),
                                       hipMemcpyDeviceToHost, io.stream));
            HIP_TRY(hipStreamSynchronize(io.stream));
            return split_check(g, dg, io.stream);
        });
}

int qldpc_decode_batch(qldpc_graph *g, const qldpc_params *p, int32_t batch, const double *llr,
                       const uint8_t *syndrome, uint8_t *bits_out, uint32_t *iters_out, uint8_t *synd_ok_out,
                       double *posterior_out) {
    if (!g) return fail(QLDPC_EINVAL, "graph is NULL");
    int rc = check_params(p);
    if (rc) return rc;
    if (batch < 0) return fail(QLDPC_EINVAL, "batch must be >= 0");
    if (batch == 0) return QLDPC_OK;
    if (!llr || !syndrome || !bits_out || !iters_out || !synd_ok_out) return fail(QLDPC_EINVAL, "NULL host buffer");
    return decode_batch_host(g, p, batch, llr, syndrome, bits_out, iters_out, synd_ok_out, posterior_out, nullptr,
                             nullptr);
}

int qldpc_decode_trace_batch(qldpc_graph *g, const qldpc_params *p, int32_t batch, const double *llr,
                             const uint8_t *syndrome, uint8_t *bits_out, uint32_t *iters_out, uint8_t *synd_ok_out,
                             double *posterior_out, uint32_t *unsat_out, double *trace_post_out) {
    if (!g) return fail(QLDPC_EINVAL, "graph is NULL");
    int rc = check_params(p);
    if (rc) return rc;
    if (batch < 0) return fail(QLDPC_EINVAL, "batch must be >= 0");
    if ((rc = trace_layout_check(g))) return rc;
    if (batch == 0) return QLDPC_OK;
    if (!llr || !syndrome || !bits_out || !iters_out || !synd_ok_out) return fail(QLDPC_EINVAL, "NULL host buffer");
    return decode_batch_host(g, p, batch, llr, syndrome, bits_out, iters_out, synd_ok_out, posterior_out, unsat_out,
                             trace_post_out);
}

int qldpc_decode_trace_batch_device(qldpc_graph *g, int32_t device, const qldpc_params *p, int32_t batch,
                                    const double *d_llr, const uint8_t *d_syndrome, uint8_t *d_bits_out,
                                    uint32_t *d_iters_out, uint8_t *d_synd_ok_out, double *d_posterior_out,
                                    uint32_t *d_unsat_out, double *d_trace_post_out, void *stream) {
    if (!g) return fail(QLDPC_EINVAL, "graph is NULL");
    int rc = check_params(p);
    if (rc) return rc;
    if (batch < 0) return fail(QLDPC_EINVAL, "batch must be >= 0");
    if ((rc = trace_layout_check(g))) return rc;
    if (batch == 0) return QLDPC_OK;
    if (!d_llr || !d_syndrome || !d_bits_out || !d_iters_out || !d_synd_ok_out)
        return fail(QLDPC_EINVAL, "NULL device buffer");
    DeviceGraph *dg = find_dev(g, device);
    if (!dg) return fail(QLDPC_EINVAL, "graph does not live on that device");
    DeviceScope ds;
    if ((rc = ds.enter(device))) return rc;
    return decode_on(g, dg, p, batch, d_llr, d_syndrome, d_bits_out, d_iters_out, d_synd_ok_out, d_posterior_out,
                     (hipStream_t)stream, false, nullptr, nullptr, d_unsat_out, d_trace_post_out);
}

int qldpc_build_frames_device(qldpc_graph *g, int32_t device, int32_t batch, const uint8_t *d_alice,
                              const uint8_t *d_bob, const double *d_log_p, double *d_llr, uint8_t *d_syndrome,
                              void *stream) {
    if (!g) return fail(QLDPC_EINVAL, "graph is NULL");
    if (batch < 0) return fail(QLDPC_EINVAL, "batch must be >= 0");
    if (batch > 0 && (!d_alice || !d_bob || !d_log_p || !d_llr || !d_syndrome))
        return fail(QLDPC_EINVAL, "NULL device buffer");
    DeviceGraph *dg = find_dev(g, device);
    if (!dg) return fail(QLDPC_EINVAL, "graph does not live on that device");
    if (int r = frame_builder_fits(g, -1)) return r;
    DeviceScope ds;
    if (int r = ds.enter(device)) return r;
    hipError_t e = launch_build_frames(g->n, g->m, g->max_dc, dg->ell_col.get(), dg->row_deg.get(), batch, d_alice,
                                       d_bob, d_log_p, d_llr, d_syndrome, nullptr, nullptr, nullptr, nullptr,
                                       (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "build_frames");
    return QLDPC_OK;
}

int qldpc_keys_match_device(int32_t batch, int32_t n, const uint8_t *d_alice, const uint8_t *d_bits,
                            uint8_t *d_keys_match, void *stream) {
    if (batch < 0 || n <= 0) return fail(QLDPC_EINVAL, "bad batch / n");
    if (batch > 0 && (!d_alice || !d_bits || !d_keys_match)) return fail(QLDPC_EINVAL, "NULL device buffer");
    hipError_t e = launch_keys_match(batch, n, d_alice, d_bits, d_keys_match, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "keys_match");
    return QLDPC_OK;
}

int qldpc_selftest_math_device(int32_t fn, int32_t count, const double *d_in, double *d_out, void *stream) {
    return qldpc_selftest_math_thr_device(fn, 100.0, count, d_in, d_out, stream);
}

int qldpc_selftest_math_thr_device(int32_t fn, double thr, int32_t count, const double *d_in, double *d_out,
                                   void *stream) {
    if (fn < 0 || fn > 9 || count < 0) return fail(QLDPC_EINVAL, "fn must be 0..9, count >= 0");
    if (!(thr > 0.)) return fail(QLDPC_EINVAL, "threshold must be > 0");
    if (count > 0 && (!d_in || !d_out)) return fail(QLDPC_EINVAL, "NULL device buffer");
    hipError_t e = launch_math_selftest(fn, spa_clip(true, thr), count, d_in, d_out, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "math_selftest");
    return QLDPC_OK;
}

int qldpc_qkd_ldpc_batch_device(qldpc_graph *g, int32_t device, const qldpc_params *p, int32_t batch,
                                const uint8_t *d_alice, const uint8_t *d_bob, const double *d_log_p,
                                double *d_llr_ws, uint8_t *d_synd_ws, uint8_t *d_bits_out, uint32_t *d_iters_out,
                                uint8_t *d_synd_ok_out, uint8_t *d_keys_match_out, void *stream) {
    if (!g) return fail(QLDPC_EINVAL, "graph is NULL");
    int rc = check_params(p);
    if (rc) return rc;
    if (batch < 0) return fail(QLDPC_EINVAL, "batch must be >= 0");
    if (batch > 0 && (!d_alice || !d_bob || !d_log_p || !d_synd_ws || !d_bits_out || !d_iters_out || !d_synd_ok_out))
        return fail(QLDPC_EINVAL, "NULL device buffer");
    DeviceGraph *dg = find_dev(g, device);
    if (!dg) return fail(QLDPC_EINVAL, "graph does not live on that device");
    if (batch == 0) return QLDPC_OK;
    DeviceScope ds;
    if ((rc = ds.enter(device))) return rc;
    return qkd_ldpc_window(g, dg, nullptr, p, batch, d_alice, d_bob, nullptr, nullptr, d_log_p, nullptr, d_llr_ws,
                           d_synd_ws, d_bits_out, d_iters_out, d_synd_ok_out, d_keys_match_out, (hipStream_t)stream);
}

// ---- rate adaptation: the plan on the graph's devices ---------------------------
int qldpc_rate_plan_create(qldpc_graph *g, int32_t n_punct, const int32_t *punctured, int32_t n_short,
                           const int32_t *shortened, qldpc_rate_plan **out) {
    if (!g || !out) return fail(QLDPC_EINVAL, "graph / out is NULL");
    *out = nullptr;
    if (n_punct < 0 || n_short < 0 || n_punct + n_short > g->n || (n_punct && !punctured) || (n_short && !shortened))
        return fail(QLDPC_EINVAL, "bad punctured / shortened lists");
    std::vector<uint8_t> cls(g->n, 0);
    std::vector<int32_t> src(g->n, 0);
    for (int i = 0; i < n_punct; ++i) {
        if (punctured[i] < 0 || punctured[i] >= g->n || (i && punctured[i] <= punctured[i - 1]))
            return fail(QLDPC_EINVAL, "punctured positions must be ascending and in [0, n)");
        cls[punctured[i]] = 1;
        src[punctured[i]] = i;
    }
    for (int i = 0; i < n_short; ++i) {
        if (shortened[i] < 0 || shortened[i] >= g->n || (i && shortened[i] <= shortened[i - 1]))
            return fail(QLDPC_EINVAL, "shortened positions must be ascending and in [0, n)");
        if (cls[shortened[i]]) return fail(QLDPC_EINVAL, "a position is both punctured and shortened");
        cls[shortened[i]] = 2;
    }
    int key = 0;
    for (int i = 0; i < g->n; ++i)
        if (cls[i] == 0) src[i] = key++;
    auto plan = std::make_unique<qldpc_rate_plan>();
    plan->n_punct = n_punct;
    plan->n_short = n_short;
    est_row_table(*g, cls.data(), plan->est);  // once per (graph, plan): the error estimate's row table
    plan->adjacency = g->adjacency;
    plan->cls = cls;
    DeviceScope restore;  // (a host-only graph: the plan lives on no device, and none is touched)
    if (int rc = g->devs.empty() ? QLDPC_OK : restore.save()) return rc;
    for (auto &dg : g->devs) {
        HIP_TRY(hipSetDevice(dg->device));
        qldpc_rate_plan::Dev d;
        d.device = dg->device;
        int rc;
        if ((rc = d.cls.upload(cls)) || (rc = d.src.upload(src)) || (rc = d.row_d.upload(plan->est.row_d))) return rc;
        plan->devs.push_back(std::move(d));
    }
    *out = plan.release();
    return QLDPC_OK;
}

void qldpc_rate_plan_destroy(qldpc_rate_plan *plan) { delete plan; }

namespace {
// The generator workspace of the _device entries, one per (device, stream),
// kept across calls so a stream-pipelined caller's launches stay asynchronous
// (grown, never shrunk; growing drains the device before freeing the old one).
// Process lifetime: raw pointers, never released.  A static destructor must not
// call into the HIP runtime, which may already be gone at exit.
std::mutex g_tws_mu;
std::map<std::pair<int, hipStream_t>, std::pair<uint32_t *, size_t>> g_tws;
hipError_t trial_workspace(hipStream_t s, size_t words, uint32_t **out) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    std::lock_guard<std::mutex> lk(g_tws_mu);
    auto &w = g_tws[{dev, s}];
    if (w.second < words) {
        if (w.first) {
            if ((e = hipDeviceSynchronize()) != hipSuccess) return e;
            (void)hipFree(w.first);
            w = {nullptr, 0};
        }
        if ((e = hipMalloc(&w.first, std::max<size_t>(words, 1) * sizeof(uint32_t))) != hipSuccess) return e;
        w.second = words;
    }
    *out = w.first;
    return hipSuccess;
}
}  // namespace

int qldpc_trials_rate_adapt_device(int32_t n, double qber, int32_t batch, const uint64_t *d_seeds, uint64_t seed_add,
                                   int32_t n_punct, uint8_t *d_alice, uint8_t *d_bob, uint8_t *d_punct_alice,
                                   uint8_t *d_punct_bob, double *accurate_qber_out, void *stream) {
    if (n_punct < 0 || (n_punct > 0 && batch > 0 && (!d_punct_alice || !d_punct_bob)))
        return fail(QLDPC_EINVAL, "bad n_punct / NULL punctured-draw buffers");
    if (n <= 0 || batch < 0) return fail(QLDPC_EINVAL, "n must be > 0 and batch >= 0");
    const uint64_t n_err = (uint64_t)((double)n * qber);
    if (n_err == 0) return fail(QLDPC_EINVAL, "Key size '" + std::to_string(n) + "' is too small for QBER.");
    if (n_err > (uint64_t)n) return fail(QLDPC_EINVAL, "QBER must be <= 1");
    if (accurate_qber_out) *accurate_qber_out = (double)n_err / (double)n;
    if (batch == 0) return QLDPC_OK;
    if (!d_seeds || !d_alice || !d_bob) return fail(QLDPC_EINVAL, "NULL device buffer");
    const hipStream_t s = (hipStream_t)stream;
    uint32_t *scratch = nullptr;
    HIP_TRY(trial_workspace(s, trials_scratch_words(n, n_err, n_punct, batch), &scratch));
    hipError_t e = launch_trials(n, n_err, batch, d_seeds, seed_add, d_alice, d_bob, scratch, n_punct, d_punct_alice,
                                 d_punct_bob, s);
    if (e != hipSuccess) return hip_fail(e, "trials_rate_adapt");
    return QLDPC_OK;
}

int qldpc_build_frames_rate_adapt_device(qldpc_graph *g, const qldpc_rate_plan *plan, int32_t device, int32_t batch,
                                         const uint8_t *d_alice, const uint8_t *d_bob, const uint8_t *d_punct_alice,
                                         const uint8_t *d_punct_bob, const double *d_log_p, uint8_t *d_alice_ext,
                                         double *d_llr, uint8_t *d_syndrome, void *stream) {
    if (!g || !plan) return fail(QLDPC_EINVAL, "graph / plan is NULL");
    if (batch < 0) return fail(QLDPC_EINVAL, "batch must be >= 0");
    if (batch > 0 && (!d_alice || !d_bob || !d_log_p || !d_alice_ext || !d_llr || !d_syndrome ||
                      (plan->n_punct && (!d_punct_alice || !d_punct_bob))))
        return fail(QLDPC_EINVAL, "NULL device buffer");
    DeviceGraph *dg = find_dev(g, device);
    const qldpc_rate_plan::Dev *pd = plan_dev(plan, device);
    if (!dg || !pd) return fail(QLDPC_EINVAL, "graph / plan does not live on that device");
    if (int r = frame_builder_fits(g, plan->n_punct)) return r;
    DeviceScope ds;
    if (int r = ds.enter(device)) return r;
    hipError_t e = launch_build_frames_ra(g->n, g->m, dg->ell_col.get(), dg->row_deg.get(), pd->cls.get(),
                                          pd->src.get(), plan->n_punct, batch, d_alice, d_bob, d_punct_alice,
                                          d_punct_bob, d_log_p, d_alice_ext, d_llr, d_syndrome, nullptr, nullptr,
                                          nullptr, nullptr, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "build_frames_rate_adapt");
    return QLDPC_OK;
}

int qldpc_qkd_ldpc_rate_adapt_batch_device(qldpc_graph *g, const qldpc_rate_plan *plan, int32_t device,
                                           const qldpc_params *p, int32_t batch, const uint8_t *d_alice,
                                           const uint8_t *d_bob, const uint8_t *d_punct_alice,
                                           const uint8_t *d_punct_bob, const double *d_log_p, uint8_t *d_alice_ext,
                                           double *d_llr_ws, uint8_t *d_synd_ws, uint8_t *d_bits_out,
                                           uint32_t *d_iters_out, uint8_t *d_synd_ok_out, uint8_t *d_keys_match_out,
                                           void *stream) {
    if (!g || !plan) return fail(QLDPC_EINVAL, "graph / plan is NULL");
    int rc = check_params(p);
    if (rc) return rc;
    if (batch < 0) return fail(QLDPC_EINVAL, "batch must be >= 0");
    if (batch == 0) return QLDPC_OK;
    if (!d_alice || !d_bob || !d_log_p || !d_alice_ext || !d_synd_ws || !d_bits_out || !d_iters_out ||
        !d_synd_ok_out || (plan->n_punct && (!d_punct_alice || !d_punct_bob)))
        return fail(QLDPC_EINVAL, "NULL device buffer");
    DeviceGraph *dg = find_dev(g, device);
    if (!dg) return fail(QLDPC_EINVAL, "graph does not live on that device");
    DeviceScope ds;
    if ((rc = ds.enter(device))) return rc;
    return qkd_ldpc_window(g, dg, plan, p, batch, d_alice, d_bob, d_punct_alice, d_punct_bob, d_log_p, d_alice_ext,
                           d_llr_ws, d_synd_ws, d_bits_out, d_iters_out, d_synd_ok_out, d_keys_match_out,
                           (hipStream_t)stream);
}

// ---- two parties: Alice's syndromes, Bob's decode from his own key ---------------
// Argument checks, in this order wherever the step applies: NULL graph, the
// parameters, batch < 0, batch == 0 (OK), NULL buffers (and the plan the
// extract entry needs), the plan on the device, the device, the LDS fit.
// Through batch == 0 no device is touched.
static bool fill_missing(const qldpc_rate_plan *plan, const uint8_t *fill) {
    return plan && plan->n_punct > 0 && !fill;
}

int qldpc_syndrome_batch_device(qldpc_graph *g, const qldpc_rate_plan *plan, int32_t device, int32_t batch,
                                const uint8_t *d_key, const uint8_t *d_punct_fill, uint8_t *d_key_ext_out,
                                uint8_t *d_syndrome_out, void *stream) {
    if (!g) return fail(QLDPC_EINVAL, "graph is NULL");
    if (batch < 0) return fail(QLDPC_EINVAL, "batch must be >= 0");
    if (batch == 0) return QLDPC_OK;
    if (!d_key || !d_syndrome_out || fill_missing(plan, d_punct_fill)) return fail(QLDPC_EINVAL, "NULL device buffer");
    const qldpc_rate_plan::Dev *pd = plan ? plan_dev(plan, device) : nullptr;
    if (plan && !pd) return fail(QLDPC_EINVAL, "rate plan does not live on that device");
    DeviceGraph *dg = find_dev(g, device);
    if (!dg) return fail(QLDPC_EINVAL, "graph does not live on that device");
    if (int r = party_fits(g, true, plan ? plan->n_punct : -1)) return r;
    DeviceScope ds;
    if (int r = ds.enter(device)) return r;
    const hipError_t e = launch_alice_syndrome(g->n, g->m, dg->ell_col.get(), dg->row_deg.get(),
                                               pd ? pd->cls.get() : nullptr, pd ? pd->src.get() : nullptr,
                                               plan ? plan->n_punct : 0, batch, d_key, d_punct_fill, d_key_ext_out,
                                               d_syndrome_out, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "alice_syndrome");
    return QLDPC_OK;
}

int qldpc_reconcile_batch_device(qldpc_graph *g, const qldpc_rate_plan *plan, int32_t device, const qldpc_params *p,
                                 int32_t batch, const uint8_t *d_key, const double *d_log_p,
                                 const uint8_t *d_syndrome, double *d_llr_ws, uint8_t *d_bits_out,
                                 uint32_t *d_iters_out, uint8_t *d_synd_ok_out, double *d_posterior_out,
                                 void *stream) {
    if (!g) return fail(QLDPC_EINVAL, "graph is NULL");
    int rc = check_params(p);
    if (rc) return rc;
    if (batch < 0) return fail(QLDPC_EINVAL, "batch must be >= 0");
    if (batch == 0) return QLDPC_OK;
    if (!d_key || !d_log_p || !d_syndrome || !d_bits_out || !d_iters_out || !d_synd_ok_out)
        return fail(QLDPC_EINVAL, "NULL device buffer");
    const qldpc_rate_plan::Dev *pd = plan ? plan_dev(plan, device) : nullptr;
    if (plan && !pd) return fail(QLDPC_EINVAL, "rate plan does not live on that device");
    DeviceGraph *dg = find_dev(g, device);
    if (!dg) return fail(QLDPC_EINVAL, "graph does not live on that device");
    if ((rc = party_fits(g, false, -1))) return rc;
    DeviceScope ds;
    if ((rc = ds.enter(device))) return rc;
    return reconcile_window(g, dg, pd, p, batch, d_key, d_log_p, d_syndrome, d_llr_ws, d_bits_out, d_iters_out,
                            d_synd_ok_out, d_posterior_out, (hipStream_t)stream);
}

int qldpc_extract_key_device(qldpc_graph *g, const qldpc_rate_plan *plan, int32_t device, int32_t batch,
                             const uint8_t *d_bits, uint8_t *d_key_out, void *stream) {
    if (!g) return fail(QLDPC_EINVAL, "graph is NULL");
    if (batch < 0) return fail(QLDPC_EINVAL, "batch must be >= 0");
    if (batch == 0) return QLDPC_OK;
    if (!plan) return fail(QLDPC_EINVAL, "plan is NULL");
    if (!d_bits || !d_key_out) return fail(QLDPC_EINVAL, "NULL device buffer");
    const qldpc_rate_plan::Dev *pd = plan_dev(plan, device);
    if (!pd) return fail(QLDPC_EINVAL, "rate plan does not live on that device");
    if (!find_dev(g, device)) return fail(QLDPC_EINVAL, "graph does not live on that device");
    DeviceScope ds;
    if (int r = ds.enter(device)) return r;
    const hipError_t e = launch_extract_key(g->n, g->n - plan->n_punct - plan->n_short, pd->cls.get(), pd->src.get(),
                                            batch, d_bits, d_key_out, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "extract_key");
    return QLDPC_OK;
}

// The host entries need the plan on every device of the graph (each shard reads its own replica).
static int plan_on_every_device(const qldpc_graph *g, const qldpc_rate_plan *plan) {
    if (!plan) return QLDPC_OK;
    for (auto &dg : g->devs)
        if (!plan_dev(plan, dg->device)) return fail(QLDPC_EINVAL, "rate plan does not live on every device of the graph");
    return QLDPC_OK;
}

int qldpc_syndrome_batch(qldpc_graph *g, const qldpc_rate_plan *plan, int32_t batch, const uint8_t *key,
                         const uint8_t *punct_fill, uint8_t *key_ext_out, uint8_t *syndrome_out) {
    if (!g) return fail(QLDPC_EINVAL, "graph is NULL");
    if (batch < 0) return fail(QLDPC_EINVAL, "batch must be >= 0");
    if (batch == 0) return QLDPC_OK;
    if (!key || !syndrome_out || fill_missing(plan, punct_fill)) return fail(QLDPC_EINVAL, "NULL host buffer");
    int rc = plan_on_every_device(g, plan);
    if (rc) return rc;
    if (g->devs.empty()) return fail(QLDPC_EINVAL, "a host-only graph cannot compute syndromes on a device");
    if ((rc = party_fits(g, true, plan ? plan->n_punct : -1))) return rc;
    const size_t n = (size_t)g->n, m = (size_t)g->m, np = plan ? (size_t)plan->n_punct : 0;
    return for_each_shard(
        g, batch, "a host-only graph cannot compute syndromes on a device",
        [&](DeviceGraph *dg, HostIO &io, int f0, int nb) -> int {
            if (int r = io.reserve((size_t)nb, n, m, false, false, true)) return r;
            const qldpc_rate_plan::Dev *pd = plan ? plan_dev(plan, dg->device) : nullptr;
            // Alice's fill and her extended key, for this call alone (allocated before anything is enqueued)
            DevBuf<uint8_t> d_fill, d_ext;
            if (int r = np ? d_fill.alloc((size_t)nb * np) : QLDPC_OK) return r;
            if (int r = (plan && key_ext_out) ? d_ext.alloc((size_t)nb * n) : QLDPC_OK) return r;
            auto enqueue = [&]() -> int {
                HIP_TRY(hipMemcpyAsync(io.key.get(), key + f0 * n, nb * n, hipMemcpyHostToDevice, io.stream));
                if (np)
                    HIP_TRY(hipMemcpyAsync(d_fill.get(), punct_fill + f0 * np, nb * np, hipMemcpyHostToDevice, io.stream));
                HIP_TRY(launch_alice_syndrome(g->n, g->m, dg->ell_col.get(), dg->row_deg.get(),
                                              pd ? pd->cls.get() : nullptr, pd ? pd->src.get() : nullptr, (int)np, nb,
                                              io.key.get(), d_fill.get(), d_ext.get(), io.synd.get(), io.stream));
                HIP_TRY(hipMemcpyAsync(syndrome_out + f0 * m, io.synd.get(), nb * m, hipMemcpyDeviceToHost, io.stream));
                if (plan && key_ext_out)  // (no plan: the key is the frame, nothing is written)
                    HIP_TRY(hipMemcpyAsync(key_ext_out + f0 * n, d_ext.get(), nb * n, hipMemcpyDeviceToHost, io.stream));
                return QLDPC_OK;
            };
            const int r = enqueue();
            const hipError_t e = hipStreamSynchronize(io.stream);  // nothing of this call stays in flight
            if (r) return r;
            if (e != hipSuccess) return hip_fail(e, "syndrome_batch");
            return QLDPC_OK;
        });
}

int qldpc_reconcile_batch(qldpc_graph *g, const qldpc_rate_plan *plan, const qldpc_params *p, int32_t batch,
                          const uint8_t *key, const double *log_p, const uint8_t *syndrome, uint8_t *bits_out,
                          uint32_t *iters_out, uint8_t *synd_ok_out, double *posterior_out) {
    if (!g) return fail(QLDPC_EINVAL, "graph is NULL");
    int rc = check_params(p);
    if (rc) return rc;
    if (batch < 0) return fail(QLDPC_EINVAL, "batch must be >= 0");
    if (batch == 0) return QLDPC_OK;
    if (!key || !log_p || !syndrome || !bits_out || !iters_out || !synd_ok_out)
        return fail(QLDPC_EINVAL, "NULL host buffer");
    if ((rc = plan_on_every_device(g, plan))) return rc;
    if (g->devs.empty()) return fail(QLDPC_EINVAL, "a host-only graph cannot decode");
    if ((rc = party_fits(g, false, -1))) return rc;
    const size_t n = (size_t)g->n, m = (size_t)g->m;
    return for_each_shard(
        g, batch, "a host-only graph cannot decode", [&](DeviceGraph *dg, HostIO &io, int f0, int nb) -> int {
            if (int r = io.reserve((size_t)nb, n, m, false, true, true)) return r;
            const qldpc_rate_plan::Dev *pd = plan ? plan_dev(plan, dg->device) : nullptr;
            auto enqueue = [&]() -> int {
                HIP_TRY(hipMemcpyAsync(io.key.get(), key + f0 * n, nb * n, hipMemcpyHostToDevice, io.stream));
                HIP_TRY(hipMemcpyAsync(io.logp.get(), log_p + f0, nb * sizeof(double), hipMemcpyHostToDevice, io.stream));
                HIP_TRY(hipMemcpyAsync(io.synd.get(), syndrome + f0 * m, nb * m, hipMemcpyHostToDevice, io.stream));
                if (int r = reconcile_window(g, dg, pd, p, nb, io.key.get(), io.logp.get(), io.synd.get(), nullptr,
                                             io.bits.get(), io.iters.get(), io.ok.get(),
                                             posterior_out ? io.post.get() : nullptr, io.stream))
                    return r;
                HIP_TRY(hipMemcpyAsync(bits_out + f0 * n, io.bits.get(), nb * n, hipMemcpyDeviceToHost, io.stream));
                HIP_TRY(hipMemcpyAsync(iters_out + f0, io.iters.get(), nb * sizeof(uint32_t), hipMemcpyDeviceToHost,
                                       io.stream));
                HIP_TRY(hipMemcpyAsync(synd_ok_out + f0, io.ok.get(), nb, hipMemcpyDeviceToHost, io.stream));
                if (posterior_out)
                    HIP_TRY(hipMemcpyAsync(posterior_out + f0 * n, io.post.get(), nb * n * sizeof(double),
                                           hipMemcpyDeviceToHost, io.stream));
                return QLDPC_OK;
            };
            const int r = enqueue();
            const hipError_t e = hipStreamSynchronize(io.stream);  // nothing of this call stays in flight
            if (r) return r;
            if (e != hipSuccess) return hip_fail(e, "reconcile_batch");
            return split_check(g, dg, io.stream);
        });
}

// ---- error estimation at the reconciliation stage ----------------------------------
// Argument checks, in the two-party order: NULL graph, batch < 0, batch == 0
// (OK), NULL buffers, the q bounds (when something is solved), the plan's
// graph and R == 0, the plan on the device, the device, the LDS fit.
namespace {

const EstTable *est_table(const qldpc_graph *g, const qldpc_rate_plan *plan) { return plan ? &plan->est : &g->est; }

int est_plan_check(const qldpc_graph *g, const qldpc_rate_plan *plan) {
    if (plan && plan->adjacency != g->adjacency)
        return fail(QLDPC_EINVAL, "the rate plan was created for a graph of another adjacency: its row table does not apply");
    return QLDPC_OK;
}

int est_bounds_check(double q_min, double q_max) {
    if (!(q_min > 0.0) || !(q_max < 0.5) || !(q_min <= q_max))  // (NaN fails each)
        return fail(QLDPC_EINVAL, "the estimate's bounds must satisfy 0 < q_min <= q_max < 0.5");
    return QLDPC_OK;
}

int est_rows_check(const EstTable *e) {
    if (e->informative == 0)
        return fail(QLDPC_EINVAL, "no informative rows: every check row has a punctured neighbour or only shortened ones");
    return QLDPC_OK;
}

int est_fits(const qldpc_graph *g, bool with_plan) {
    const size_t lds = syndrome_weight_lds(g->n, with_plan);
    if (lds <= LDS_MAX_BYTES) return QLDPC_OK;
    return fail(QLDPC_EUNSUP, "n = " + std::to_string(g->n) + ": the syndrome-weight kernel keeps the key in LDS (" +
                                  std::to_string(lds) + " bytes > " + std::to_string(LDS_MAX_BYTES) + ")");
}

int est_classes_fit(const EstTable *e) {
    if (e->degree.size() <= (size_t)EST_MAX_CLASSES) return QLDPC_OK;
    return fail(QLDPC_EUNSUP, std::to_string(e->degree.size()) + " degree classes: the solve kernel takes at most " +
                                  std::to_string(EST_MAX_CLASSES) + " (qldpc_qber_from_weight solves any number)");
}

// The weights, then (qber or log_p wanted) the solve, on `s`; the current
// device is dg's.  d_weight NULL: the weights go to the stream's workspace.
int estimate_window(qldpc_graph *g, DeviceGraph *dg, const qldpc_rate_plan::Dev *pd, const EstTable *e, int batch,
                    const uint8_t *d_key, const uint8_t *d_synd, double q_min, double q_max, int32_t *d_weight,
                    double *d_qber, double *d_log_p, hipStream_t s) {
    if (!d_weight) {
        std::lock_guard<std::mutex> lk(dg->mu);
        Workspace *w = workspace(dg, s);
        if (int r = grow(w->est_frames, (size_t)batch, s, [&] { return w->est_weight.alloc((size_t)batch); })) return r;
        d_weight = w->est_weight.get();
    }
    HIP_TRY(launch_syndrome_weight(g->n, g->m, dg->ell_col.get(), dg->row_deg.get(),
                                   pd ? pd->row_d.get() : dg->row_deg.get(), pd ? pd->cls.get() : nullptr,
                                   pd ? pd->src.get() : nullptr, batch, d_key, d_synd, d_weight, s));
    if (d_qber || d_log_p)
        HIP_TRY(launch_estimate_solve(batch, (int)e->degree.size(), e->degree.data(), e->rows.data(), d_weight, q_min,
                                      q_max, d_qber, d_log_p, s));
    return QLDPC_OK;
}

}  // namespace

int qldpc_estimate_classes(qldpc_graph *g, const qldpc_rate_plan *plan, int32_t cap, int32_t *n_classes,
                           int32_t *degree_out, int32_t *rows_out) {
    if (!g) return fail(QLDPC_EINVAL, "graph is NULL");
    if (cap < 0 || !n_classes || (cap > 0 && (!degree_out || !rows_out)))
        return fail(QLDPC_EINVAL, "cap must be >= 0 and the outputs not NULL");
    if (int r = est_plan_check(g, plan)) return r;
    const EstTable *e = est_table(g, plan);
    *n_classes = (int32_t)e->degree.size();
    for (size_t c = 0; c < e->degree.size() && c < (size_t)cap; ++c) {
        degree_out[c] = e->degree[c];
        rows_out[c] = e->rows[c];
    }
    return QLDPC_OK;
}

int qldpc_qber_from_weight(qldpc_graph *g, const qldpc_rate_plan *plan, int32_t count, const int64_t *weight,
                           int64_t frames_per_weight, double q_min, double q_max, double *qber_out,
                           double *log_p_out) {
    if (!g) return fail(QLDPC_EINVAL, "graph is NULL");
    if (count < 0) return fail(QLDPC_EINVAL, "count must be >= 0");
    if (count == 0) return QLDPC_OK;
    if (!weight || !qber_out) return fail(QLDPC_EINVAL, "NULL host buffer");
    if (frames_per_weight < 1) return fail(QLDPC_EINVAL, "frames_per_weight must be >= 1");
    int rc;
    if ((rc = est_bounds_check(q_min, q_max)) || (rc = est_plan_check(g, plan))) return rc;
    const EstTable *e = est_table(g, plan);
    if ((rc = est_rows_check(e))) return rc;
    if (frames_per_weight > (INT64_MAX >> 1) / e->informative)
        return fail(QLDPC_EINVAL, "frames_per_weight is too large");
    const int64_t most = frames_per_weight * e->informative;
    for (int32_t i = 0; i < count; ++i)
        if (weight[i] < 0 || weight[i] > most)
            return fail(QLDPC_EINVAL, "a weight lies outside [0, frames_per_weight * informative rows]");
    const ql_exact::EstClasses cl = {(int32_t)e->degree.size(), e->degree.data(), e->rows.data()};
    for (int32_t i = 0; i < count; ++i) {
        qber_out[i] = ql_exact::est_qber(cl, weight[i], frames_per_weight, q_min, q_max);
        if (log_p_out) log_p_out[i] = ql_exact::est_log_p(qber_out[i]);
    }
    return QLDPC_OK;
}

int qldpc_estimate_qber_device(qldpc_graph *g, const qldpc_rate_plan *plan, int32_t device, int32_t batch,
                               const uint8_t *d_key, const uint8_t *d_syndrome, double q_min, double q_max,
                               int32_t *d_weight_out, double *d_qber_out, double *d_log_p_out, void *stream) {
    if (!g) return fail(QLDPC_EINVAL, "graph is NULL");
    if (batch < 0) return fail(QLDPC_EINVAL, "batch must be >= 0");
    if (batch == 0) return QLDPC_OK;
    if (!d_key || !d_syndrome || (!d_weight_out && !d_qber_out && !d_log_p_out))
        return fail(QLDPC_EINVAL, "NULL device buffer");
    const bool solve = d_qber_out || d_log_p_out;
    int rc;
    if (solve && (rc = est_bounds_check(q_min, q_max))) return rc;
    if ((rc = est_plan_check(g, plan))) return rc;
    const EstTable *e = est_table(g, plan);
    if ((rc = est_rows_check(e))) return rc;
    const qldpc_rate_plan::Dev *pd = plan ? plan_dev(plan, device) : nullptr;
    if (plan && !pd) return fail(QLDPC_EINVAL, "rate plan does not live on that device");
    DeviceGraph *dg = find_dev(g, device);
    if (!dg) return fail(QLDPC_EINVAL, "graph does not live on that device");
    if ((rc = est_fits(g, plan != nullptr)) || (solve && (rc = est_classes_fit(e)))) return rc;
    DeviceScope ds;
    if ((rc = ds.enter(device))) return rc;
    return estimate_window(g, dg, pd, e, batch, d_key, d_syndrome, q_min, q_max, d_weight_out, d_qber_out, d_log_p_out,
                           (hipStream_t)stream);
}

int qldpc_corrected_errors_device(qldpc_graph *g, const qldpc_rate_plan *plan, int32_t device, int32_t batch,
                                  const uint8_t *d_key, const uint8_t *d_bits, int32_t *d_errors_out, void *stream) {
    if (!g) return fail(QLDPC_EINVAL, "graph is NULL");
    if (batch < 0) return fail(QLDPC_EINVAL, "batch must be >= 0");
    if (batch == 0) return QLDPC_OK;
    if (!d_key || !d_bits || !d_errors_out) return fail(QLDPC_EINVAL, "NULL device buffer");
    const qldpc_rate_plan::Dev *pd = plan ? plan_dev(plan, device) : nullptr;
    if (plan && !pd) return fail(QLDPC_EINVAL, "rate plan does not live on that device");
    if (!find_dev(g, device)) return fail(QLDPC_EINVAL, "graph does not live on that device");
    DeviceScope ds;
    if (int r = ds.enter(device)) return r;
    HIP_TRY(launch_corrected_errors(g->n, pd ? pd->cls.get() : nullptr, pd ? pd->src.get() : nullptr, batch, d_key,
                                    d_bits, d_errors_out, (hipStream_t)stream));
    return QLDPC_OK;
}

int qldpc_estimate_qber_batch(qldpc_graph *g, const qldpc_rate_plan *plan, int32_t batch, const uint8_t *key,
                              const uint8_t *syndrome, double q_min, double q_max, int32_t *weight_out,
                              double *qber_out, double *log_p_out) {
    if (!g) return fail(QLDPC_EINVAL, "graph is NULL");
    if (batch < 0) return fail(QLDPC_EINVAL, "batch must be >= 0");
    if (batch == 0) return QLDPC_OK;
    if (!key || !syndrome || (!weight_out && !qber_out && !log_p_out)) return fail(QLDPC_EINVAL, "NULL host buffer");
    const bool solve = qber_out || log_p_out;
    int rc;
    if (solve && (rc = est_bounds_check(q_min, q_max))) return rc;
    if ((rc = est_plan_check(g, plan))) return rc;
    const EstTable *e = est_table(g, plan);
    if ((rc = est_rows_check(e)) || (rc = plan_on_every_device(g, plan))) return rc;
    if (g->devs.empty()) return fail(QLDPC_EINVAL, "a host-only graph cannot estimate on a device");
    if ((rc = est_fits(g, plan != nullptr)) || (solve && (rc = est_classes_fit(e)))) return rc;
    const size_t n = (size_t)g->n, m = (size_t)g->m;
    return for_each_shard(
        g, batch, "a host-only graph cannot estimate on a device",
        [&](DeviceGraph *dg, HostIO &io, int f0, int nb) -> int {
            if (int r = io.reserve((size_t)nb, n, m, false, false, true)) return r;
            const qldpc_rate_plan::Dev *pd = plan ? plan_dev(plan, dg->device) : nullptr;
            DevBuf<int32_t> d_w;  // for this call alone (allocated before anything is enqueued)
            DevBuf<double> d_q;
            if (int r = d_w.alloc((size_t)nb)) return r;
            if (int r = qber_out ? d_q.alloc((size_t)nb) : QLDPC_OK) return r;
            auto enqueue = [&]() -> int {
                HIP_TRY(hipMemcpyAsync(io.key.get(), key + f0 * n, nb * n, hipMemcpyHostToDevice, io.stream));
                HIP_TRY(hipMemcpyAsync(io.synd.get(), syndrome + f0 * m, nb * m, hipMemcpyHostToDevice, io.stream));
                if (int r = estimate_window(g, dg, pd, e, nb, io.key.get(), io.synd.get(), q_min, q_max, d_w.get(),
                                            d_q.get(), log_p_out ? io.logp.get() : nullptr, io.stream))
                    return r;
                if (weight_out)
                    HIP_TRY(hipMemcpyAsync(weight_out + f0, d_w.get(), nb * sizeof(int32_t), hipMemcpyDeviceToHost,
                                           io.stream));
                if (qber_out)
                    HIP_TRY(hipMemcpyAsync(qber_out + f0, d_q.get(), nb * sizeof(double), hipMemcpyDeviceToHost,
                                           io.stream));
                if (log_p_out)
                    HIP_TRY(hipMemcpyAsync(log_p_out + f0, io.logp.get(), nb * sizeof(double), hipMemcpyDeviceToHost,
                                           io.stream));
                return QLDPC_OK;
            };
            const int r = enqueue();
            const hipError_t err = hipStreamSynchronize(io.stream);  // nothing of this call stays in flight
            if (r) return r;
            if (err != hipSuccess) return hip_fail(err, "estimate_qber_batch");
            return QLDPC_OK;
        });
}

int qldpc_corrected_errors_batch(qldpc_graph *g, const qldpc_rate_plan *plan, int32_t batch, const uint8_t *key,
                                 const uint8_t *bits, int32_t *errors_out) {
    if (!g) return fail(QLDPC_EINVAL, "graph is NULL");
    if (batch < 0) return fail(QLDPC_EINVAL, "batch must be >= 0");
    if (batch == 0) return QLDPC_OK;
    if (!key || !bits || !errors_out) return fail(QLDPC_EINVAL, "NULL host buffer");
    if (int rc = plan_on_every_device(g, plan)) return rc;
    if (g->devs.empty()) return fail(QLDPC_EINVAL, "a host-only graph cannot count errors on a device");
    const size_t n = (size_t)g->n, m = (size_t)g->m;
    return for_each_shard(
        g, batch, "a host-only graph cannot count errors on a device",
        [&](DeviceGraph *dg, HostIO &io, int f0, int nb) -> int {
            if (int r = io.reserve((size_t)nb, n, m, false, false, true)) return r;
            const qldpc_rate_plan::Dev *pd = plan ? plan_dev(plan, dg->device) : nullptr;
            DevBuf<uint8_t> d_bits;  // for this call alone (allocated before anything is enqueued)
            DevBuf<int32_t> d_err;
            if (int r = d_bits.alloc((size_t)nb * n)) return r;
            if (int r = d_err.alloc((size_t)nb)) return r;
            auto enqueue = [&]() -> int {
                HIP_TRY(hipMemcpyAsync(io.key.get(), key + f0 * n, nb * n, hipMemcpyHostToDevice, io.stream));
                HIP_TRY(hipMemcpyAsync(d_bits.get(), bits + f0 * n, nb * n, hipMemcpyHostToDevice, io.stream));
                HIP_TRY(launch_corrected_errors(g->n, pd ? pd->cls.get() : nullptr, pd ? pd->src.get() : nullptr, nb,
                                                io.key.get(), d_bits.get(), d_err.get(), io.stream));
                HIP_TRY(hipMemcpyAsync(errors_out + f0, d_err.get(), nb * sizeof(int32_t), hipMemcpyDeviceToHost,
                                       io.stream));
                return QLDPC_OK;
            };
            const int r = enqueue();
            const hipError_t err = hipStreamSynchronize(io.stream);  // nothing of this call stays in flight
            if (r) return r;
            if (err != hipSuccess) return hip_fail(err, "corrected_errors_batch");
            return QLDPC_OK;
        });
}

// ---- blind reconciliation: disclosure rounds for the frames that failed ----------
// Argument checks, in the two-party order: NULL graph, the parameters,
// batch < 0, n_list outside [0, batch], n_disc outside [0, n_punct],
// n_list == 0 (OK), the plan and NULL buffers, the plan on the device, the
// device, the LDS fit.  Through n_list == 0 no device is touched.
static int check_round_counts(const qldpc_rate_plan *plan, int32_t batch /* < 0: unknown */, int32_t n_list,
                              int32_t n_disc) {
    if (n_list < 0) return fail(QLDPC_EINVAL, "n_list must be >= 0");
    if (batch >= 0 && n_list > batch) return fail(QLDPC_EINVAL, "n_list must be <= batch");
    if (n_disc < 0 || (plan && n_disc > plan->n_punct))
        return fail(QLDPC_EINVAL, "n_disc must be in [0, n_punct]");
    return QLDPC_OK;
}

int qldpc_failed_frames_device(int32_t batch, const uint8_t *d_synd_ok, int32_t *d_list_out, int32_t *d_count_out,
                               void *stream) {
    if (batch < 0) return fail(QLDPC_EINVAL, "batch must be >= 0");
    if (batch == 0) return QLDPC_OK;
    if (!d_synd_ok || !d_list_out || !d_count_out) return fail(QLDPC_EINVAL, "NULL device buffer");
    const hipError_t e = launch_failed_frames(batch, d_synd_ok, d_list_out, d_count_out, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "failed_frames");
    return QLDPC_OK;
}

int qldpc_disclose_device(qldpc_graph *g, const qldpc_rate_plan *plan, int32_t device, int32_t n_list,
                          const int32_t *d_list, const uint8_t *d_punct_fill, int32_t n_disc, const int32_t *d_disc,
                          uint8_t *d_vals_out, void *stream) {
    if (!g) return fail(QLDPC_EINVAL, "graph is NULL");
    if (int rc = check_round_counts(plan, -1, n_list, n_disc)) return rc;
    if (n_list == 0) return QLDPC_OK;
    if (!plan) return fail(QLDPC_EINVAL, "plan is NULL");
    if (!d_list || (n_disc > 0 && (!d_punct_fill || !d_disc || !d_vals_out)))
        return fail(QLDPC_EINVAL, "NULL device buffer");
    if (!plan_dev(plan, device)) return fail(QLDPC_EINVAL, "rate plan does not live on that device");
    if (!find_dev(g, device)) return fail(QLDPC_EINVAL, "graph does not live on that device");
    DeviceScope ds;
    if (int r = ds.enter(device)) return r;
    const hipError_t e = launch_disclose(plan->n_punct, n_list, d_list, d_punct_fill, n_disc, d_disc, d_vals_out,
                                         (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "disclose");
    return QLDPC_OK;
}

int qldpc_reconcile_round_device(qldpc_graph *g, const qldpc_rate_plan *plan, int32_t device, const qldpc_params *p,
                                 int32_t batch, const uint8_t *d_key, const double *d_log_p,
                                 const uint8_t *d_syndrome, int32_t n_list, const int32_t *d_list, int32_t n_disc,
                                 const int32_t *d_disc, const uint8_t *d_vals, uint8_t *d_bits_out,
                                 uint32_t *d_iters_out, uint8_t *d_synd_ok_out, double *d_posterior_out,
                                 void *stream) {
    if (!g) return fail(QLDPC_EINVAL, "graph is NULL");
    int rc = check_params(p);
    if (rc) return rc;
    if (batch < 0) return fail(QLDPC_EINVAL, "batch must be >= 0");
    if ((rc = check_round_counts(plan, batch, n_list, n_disc))) return rc;
    if (n_list == 0) return QLDPC_OK;
    if (!plan) return fail(QLDPC_EINVAL, "plan is NULL");
    if (!d_key || !d_log_p || !d_syndrome || !d_list || !d_bits_out || !d_iters_out || !d_synd_ok_out ||
        (n_disc > 0 && (!d_disc || !d_vals)))
        return fail(QLDPC_EINVAL, "NULL device buffer");
    const qldpc_rate_plan::Dev *pd = plan_dev(plan, device);
    if (!pd) return fail(QLDPC_EINVAL, "rate plan does not live on that device");
    DeviceGraph *dg = find_dev(g, device);
    if (!dg) return fail(QLDPC_EINVAL, "graph does not live on that device");
    if ((rc = round_fits(g, plan->n_punct))) return rc;
    DeviceScope ds;
    if ((rc = ds.enter(device))) return rc;
    return round_window(g, dg, pd, plan->n_punct, p, batch, d_key, d_log_p, d_syndrome, n_list, d_list, n_disc, d_disc,
                        d_vals, d_bits_out, d_iters_out, d_synd_ok_out, d_posterior_out, (hipStream_t)stream);
}

// The host entries see the list and the indices, so they check what the device
// entries leave to the caller: list entries distinct and in [0, batch), disc in
// [0, n_punct).
static int check_host_list(int32_t batch, int32_t n_list, const int32_t *list, int32_t n_punct, int32_t n_disc,
                           const int32_t *disc) {
    std::vector<bool> seen((size_t)batch, false);
    for (int j = 0; j < n_list; ++j) {
        if (list[j] < 0 || list[j] >= batch) return fail(QLDPC_EINVAL, "list names a frame outside [0, batch)");
        if (seen[list[j]]) return fail(QLDPC_EINVAL, "list names a frame twice");
        seen[list[j]] = true;
    }
    for (int i = 0; i < n_disc; ++i)
        if (disc[i] < 0 || disc[i] >= n_punct) return fail(QLDPC_EINVAL, "disc names an index outside [0, n_punct)");
    return QLDPC_OK;
}

int qldpc_disclose_batch(qldpc_graph *g, const qldpc_rate_plan *plan, int32_t batch, int32_t n_list,
                         const int32_t *list, const uint8_t *punct_fill, int32_t n_disc, const int32_t *disc,
                         uint8_t *vals_out) {
    if (!g) return fail(QLDPC_EINVAL, "graph is NULL");
    if (batch < 0) return fail(QLDPC_EINVAL, "batch must be >= 0");
    int rc = check_round_counts(plan, batch, n_list, n_disc);
    if (rc) return rc;
    if (n_list == 0) return QLDPC_OK;
    if (!plan) return fail(QLDPC_EINVAL, "plan is NULL");
    if (!list || (n_disc > 0 && (!punct_fill || !disc || !vals_out))) return fail(QLDPC_EINVAL, "NULL host buffer");
    if ((rc = check_host_list(batch, n_list, list, plan->n_punct, n_disc, disc))) return rc;
    if ((rc = plan_on_every_device(g, plan))) return rc;
    if (g->devs.empty()) return fail(QLDPC_EINVAL, "a host-only graph cannot disclose on a device");
    if (n_disc == 0) return QLDPC_OK;
    const size_t np = (size_t)plan->n_punct, nd = (size_t)n_disc;
    return for_each_shard(
        g, n_list, "a host-only graph cannot disclose on a device",
        [&](DeviceGraph *, HostIO &io, int j0, int nb) -> int {
            // only the listed frames' fill rows travel
            std::vector<uint8_t> rows((size_t)nb * np);
            for (int j = 0; j < nb; ++j)
                std::memcpy(rows.data() + (size_t)j * np, punct_fill + (size_t)list[j0 + j] * np, np);
            DevBuf<uint8_t> d_fill, d_vals;
            DevBuf<int32_t> d_disc;
            if (int r = d_fill.alloc((size_t)nb * np)) return r;
            if (int r = d_vals.alloc((size_t)nb * nd)) return r;
            if (int r = d_disc.alloc(nd)) return r;
            auto enqueue = [&]() -> int {
                HIP_TRY(hipMemcpyAsync(d_fill.get(), rows.data(), rows.size(), hipMemcpyHostToDevice, io.stream));
                HIP_TRY(hipMemcpyAsync(d_disc.get(), disc, nd * sizeof(int32_t), hipMemcpyHostToDevice, io.stream));
                HIP_TRY(launch_disclose((int)np, nb, nullptr, d_fill.get(), n_disc, d_disc.get(), d_vals.get(),
                                        io.stream));
                HIP_TRY(hipMemcpyAsync(vals_out + (size_t)j0 * nd, d_vals.get(), (size_t)nb * nd,
                                       hipMemcpyDeviceToHost, io.stream));
                return QLDPC_OK;
            };
            const int r = enqueue();
            const hipError_t e = hipStreamSynchronize(io.stream);  // nothing of this call stays in flight
            if (r) return r;
            if (e != hipSuccess) return hip_fail(e, "disclose_batch");
            return QLDPC_OK;
        });
}

int qldpc_reconcile_round_batch(qldpc_graph *g, const qldpc_rate_plan *plan, const qldpc_params *p, int32_t batch,
                                const uint8_t *key, const double *log_p, const uint8_t *syndrome, int32_t n_list,
                                const int32_t *list, int32_t n_disc, const int32_t *disc, const uint8_t *vals,
                                uint8_t *bits_out, uint32_t *iters_out, uint8_t *synd_ok_out, double *posterior_out) {
    if (!g) return fail(QLDPC_EINVAL, "graph is NULL");
    int rc = check_params(p);
    if (rc) return rc;
    if (batch < 0) return fail(QLDPC_EINVAL, "batch must be >= 0");
    if ((rc = check_round_counts(plan, batch, n_list, n_disc))) return rc;
    if (n_list == 0) return QLDPC_OK;
    if (!plan) return fail(QLDPC_EINVAL, "plan is NULL");
    if (!key || !log_p || !syndrome || !list || !bits_out || !iters_out || !synd_ok_out ||
        (n_disc > 0 && (!disc || !vals)))
        return fail(QLDPC_EINVAL, "NULL host buffer");
    if ((rc = check_host_list(batch, n_list, list, plan->n_punct, n_disc, disc))) return rc;
    if ((rc = plan_on_every_device(g, plan))) return rc;
    if (g->devs.empty()) return fail(QLDPC_EINVAL, "a host-only graph cannot decode");
    if ((rc = round_fits(g, plan->n_punct))) return rc;
    const size_t n = (size_t)g->n, m = (size_t)g->m, nd = (size_t)n_disc;
    return for_each_shard(
        g, n_list, "a host-only graph cannot decode", [&](DeviceGraph *dg, HostIO &io, int j0, int nb) -> int {
            if (int r = io.reserve((size_t)nb, n, m, false, true, true)) return r;
            const qldpc_rate_plan::Dev *pd = plan_dev(plan, dg->device);
            // only the listed frames' key rows, log_p, syndromes and disclosed bytes travel
            std::vector<uint8_t> hkey((size_t)nb * n), hsynd((size_t)nb * m), hbits((size_t)nb * n), hok((size_t)nb);
            std::vector<double> hlogp((size_t)nb), hpost(posterior_out ? (size_t)nb * n : 0);
            std::vector<uint32_t> hiters((size_t)nb);
            for (int j = 0; j < nb; ++j) {
                const size_t f = (size_t)list[j0 + j];
                std::memcpy(hkey.data() + (size_t)j * n, key + f * n, n);
                std::memcpy(hsynd.data() + (size_t)j * m, syndrome + f * m, m);
                hlogp[j] = log_p[f];
            }
            DevBuf<uint8_t> d_vals;
            DevBuf<int32_t> d_disc;
            if (int r = nd ? d_vals.alloc((size_t)nb * nd) : QLDPC_OK) return r;
            if (int r = nd ? d_disc.alloc(nd) : QLDPC_OK) return r;
            auto enqueue = [&]() -> int {
                HIP_TRY(hipMemcpyAsync(io.key.get(), hkey.data(), hkey.size(), hipMemcpyHostToDevice, io.stream));
                HIP_TRY(hipMemcpyAsync(io.logp.get(), hlogp.data(), nb * sizeof(double), hipMemcpyHostToDevice,
                                       io.stream));
                HIP_TRY(hipMemcpyAsync(io.synd.get(), hsynd.data(), hsynd.size(), hipMemcpyHostToDevice, io.stream));
                if (nd) {
                    HIP_TRY(hipMemcpyAsync(d_vals.get(), vals + (size_t)j0 * nd, (size_t)nb * nd,
                                           hipMemcpyHostToDevice, io.stream));
                    HIP_TRY(hipMemcpyAsync(d_disc.get(), disc, nd * sizeof(int32_t), hipMemcpyHostToDevice,
                                           io.stream));
                }
                if (int r = round_window(g, dg, pd, plan->n_punct, p, nb, io.key.get(), io.logp.get(), io.synd.get(),
                                         nb, nullptr, n_disc, d_disc.get(), d_vals.get(), io.bits.get(),
                                         io.iters.get(), io.ok.get(), posterior_out ? io.post.get() : nullptr,
                                         io.stream))
                    return r;
                HIP_TRY(hipMemcpyAsync(hbits.data(), io.bits.get(), hbits.size(), hipMemcpyDeviceToHost, io.stream));
                HIP_TRY(hipMemcpyAsync(hiters.data(), io.iters.get(), nb * sizeof(uint32_t), hipMemcpyDeviceToHost,
                                       io.stream));
                HIP_TRY(hipMemcpyAsync(hok.data(), io.ok.get(), nb, hipMemcpyDeviceToHost, io.stream));
                if (posterior_out)
                    HIP_TRY(hipMemcpyAsync(hpost.data(), io.post.get(), hpost.size() * sizeof(double),
                                           hipMemcpyDeviceToHost, io.stream));
                return QLDPC_OK;
            };
            const int r = enqueue();
            const hipError_t e = hipStreamSynchronize(io.stream);  // nothing of this call stays in flight
            if (r) return r;
            if (e != hipSuccess) return hip_fail(e, "reconcile_round_batch");
            if (int sc = split_check(g, dg, io.stream)) return sc;
            for (int j = 0; j < nb; ++j) {  // (distinct rows: the shards write disjoint frames)
                const size_t f = (size_t)list[j0 + j];
                std::memcpy(bits_out + f * n, hbits.data() + (size_t)j * n, n);
                iters_out[f] = hiters[j];
                synd_ok_out[f] = hok[j];
                if (posterior_out) std::memcpy(posterior_out + f * n, hpost.data() + (size_t)j * n, n * sizeof(double));
            }
            return QLDPC_OK;
        });
}

// ---- symmetric blind reconciliation: each frame's least reliable positions --------
// Argument checks, in the two-party order: NULL graph, the parameters,
// batch < 0, n_list outside [0, batch], first / count / n_disc / cap,
// n_list == 0 (OK), NULL buffers, (host entries) the list and the position
// history, count > QLDPC_SELECT_MAX, the plan on the device, the device, the
// LDS fit.  A plan is optional.  Through n_list == 0 no device is touched.
static_assert(SELECT_MAX == QLDPC_SELECT_MAX, "the header's limit is the kernel's");

static int check_window(int32_t batch /* < 0: unknown */, int32_t n_list, int32_t first, int32_t count, int32_t cap) {
    if (n_list < 0) return fail(QLDPC_EINVAL, "n_list must be >= 0");
    if (batch >= 0 && n_list > batch) return fail(QLDPC_EINVAL, "n_list must be <= batch");
    if (first < 0 || count < 0 || cap < 0 || (int64_t)first + count > cap)
        return fail(QLDPC_EINVAL, "first and count must be >= 0 with first + count <= cap");
    return QLDPC_OK;
}

static int select_unsupported(int32_t count) {
    if (count <= QLDPC_SELECT_MAX) return QLDPC_OK;
    return fail(QLDPC_EUNSUP, "count = " + std::to_string(count) + " exceeds QLDPC_SELECT_MAX (" +
                                  std::to_string(QLDPC_SELECT_MAX) + "): select in several calls");
}

static int select_fits(const qldpc_graph *g, int count) {
    const size_t lds = select_lds(g->n, count);
    if (lds <= LDS_MAX_BYTES) return QLDPC_OK;
    return fail(QLDPC_EUNSUP, "n = " + std::to_string(g->n) + ": the select kernel keeps one bit per position in LDS (" +
                                  std::to_string(lds) + " bytes > " + std::to_string(LDS_MAX_BYTES) + ")");
}

static int positions_fit(const qldpc_graph *g) {
    const size_t lds = positions_frames_lds(g->n);
    if (lds <= LDS_MAX_BYTES) return QLDPC_OK;
    return fail(QLDPC_EUNSUP, "n = " + std::to_string(g->n) + ": the positions round's frame kernel keeps the key in " +
                                  "LDS (" + std::to_string(lds) + " bytes > " + std::to_string(LDS_MAX_BYTES) + ")");
}

int qldpc_select_positions_device(qldpc_graph *g, const qldpc_rate_plan *plan, int32_t device, int32_t batch,
                                  const double *d_posterior, int32_t n_list, const int32_t *d_list, int32_t first,
                                  int32_t count, int32_t *d_pos, int32_t cap, void *stream) {
    if (!g) return fail(QLDPC_EINVAL, "graph is NULL");
    if (batch < 0) return fail(QLDPC_EINVAL, "batch must be >= 0");
    if (int rc = check_window(batch, n_list, first, count, cap)) return rc;
    if (n_list == 0) return QLDPC_OK;
    if (!d_list || (count > 0 && (!d_posterior || !d_pos))) return fail(QLDPC_EINVAL, "NULL device buffer");
    if (int rc = select_unsupported(count)) return rc;
    const qldpc_rate_plan::Dev *pd = plan ? plan_dev(plan, device) : nullptr;
    if (plan && !pd) return fail(QLDPC_EINVAL, "rate plan does not live on that device");
    if (!find_dev(g, device)) return fail(QLDPC_EINVAL, "graph does not live on that device");
    if (int rc = select_fits(g, count)) return rc;
    DeviceScope ds;
    if (int r = ds.enter(device)) return r;
    const hipError_t e = launch_select(g->n, batch, pd ? pd->cls.get() : nullptr, n_list, d_list, d_posterior, first,
                                       count, d_pos, cap, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "select_positions");
    return QLDPC_OK;
}

int qldpc_disclose_positions_device(qldpc_graph *g, const qldpc_rate_plan *plan, int32_t device, int32_t n_list,
                                    const int32_t *d_list, const uint8_t *d_ext, int64_t ext_stride,
                                    const int32_t *d_pos, int32_t cap, int32_t first, int32_t count,
                                    uint8_t *d_vals_out, void *stream) {
    if (!g) return fail(QLDPC_EINVAL, "graph is NULL");
    if (int rc = check_window(-1, n_list, first, count, cap)) return rc;
    if (ext_stride < g->n) return fail(QLDPC_EINVAL, "ext_stride must be >= n");
    if (n_list == 0) return QLDPC_OK;
    if (!d_list || (count > 0 && (!d_ext || !d_pos || !d_vals_out))) return fail(QLDPC_EINVAL, "NULL device buffer");
    if (plan && !plan_dev(plan, device)) return fail(QLDPC_EINVAL, "rate plan does not live on that device");
    if (!find_dev(g, device)) return fail(QLDPC_EINVAL, "graph does not live on that device");
    DeviceScope ds;
    if (int r = ds.enter(device)) return r;
    const hipError_t e = launch_disclose_positions(g->n, n_list, d_list, d_ext, (size_t)ext_stride, d_pos, cap, first,
                                                   count, d_vals_out, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "disclose_positions");
    return QLDPC_OK;
}

int qldpc_reconcile_positions_round_device(qldpc_graph *g, const qldpc_rate_plan *plan, int32_t device,
                                           const qldpc_params *p, int32_t batch, const uint8_t *d_key,
                                           const double *d_log_p, const uint8_t *d_syndrome, int32_t n_list,
                                           const int32_t *d_list, int32_t n_disc, const int32_t *d_pos, int32_t cap,
                                           const uint8_t *d_vals, uint8_t *d_bits_out, uint32_t *d_iters_out,
                                           uint8_t *d_synd_ok_out, double *d_posterior_out, void *stream) {
    if (!g) return fail(QLDPC_EINVAL, "graph is NULL");
    int rc = check_params(p);
    if (rc) return rc;
    if (batch < 0) return fail(QLDPC_EINVAL, "batch must be >= 0");
    if ((rc = check_window(batch, n_list, 0, n_disc, cap))) return rc;
    if (n_list == 0) return QLDPC_OK;
    if (!d_key || !d_log_p || !d_syndrome || !d_list || !d_bits_out || !d_iters_out || !d_synd_ok_out ||
        (n_disc > 0 && (!d_pos || !d_vals)))
        return fail(QLDPC_EINVAL, "NULL device buffer");
    const qldpc_rate_plan::Dev *pd = plan ? plan_dev(plan, device) : nullptr;
    if (plan && !pd) return fail(QLDPC_EINVAL, "rate plan does not live on that device");
    DeviceGraph *dg = find_dev(g, device);
    if (!dg) return fail(QLDPC_EINVAL, "graph does not live on that device");
    if ((rc = positions_fit(g))) return rc;
    DeviceScope ds;
    if ((rc = ds.enter(device))) return rc;
    return round_window(g, dg, pd, plan ? plan->n_punct : 0, p, batch, d_key, d_log_p, d_syndrome, n_list, d_list, n_disc,
                        nullptr, d_vals, d_bits_out, d_iters_out, d_synd_ok_out, d_posterior_out, (hipStream_t)stream,
                        true, d_pos, cap);
}

// The host entries see the list and the positions, so they check what the
// device entries leave to the caller: list entries distinct and in [0, batch);
// each listed frame's pos[f][0 .. n_hist) distinct and in [0, n); count within
// the frame's candidates.
static int check_host_positions(const qldpc_graph *g, const qldpc_rate_plan *plan, int32_t batch, int32_t n_list,
                                const int32_t *list, const int32_t *pos, int32_t cap, int32_t n_hist,
                                int32_t count /* < 0: nothing is selected */) {
    std::vector<bool> seen((size_t)batch, false);
    for (int j = 0; j < n_list; ++j) {
        if (list[j] < 0 || list[j] >= batch) return fail(QLDPC_EINVAL, "list names a frame outside [0, batch)");
        if (seen[list[j]]) return fail(QLDPC_EINVAL, "list names a frame twice");
        seen[list[j]] = true;
    }
    if (count >= 0 && count > g->n - (plan ? plan->n_short : 0) - n_hist)
        return fail(QLDPC_EINVAL, "count exceeds the frame's candidates (n - n_short - first)");
    std::vector<int32_t> stamp(n_hist > 0 ? (size_t)g->n : 0, -1);
    for (int j = 0; j < n_list && n_hist > 0; ++j) {
        const int32_t *row = pos + (size_t)list[j] * (size_t)cap;
        for (int i = 0; i < n_hist; ++i) {
            if (row[i] < 0 || row[i] >= g->n) return fail(QLDPC_EINVAL, "pos names a position outside [0, n)");
            if (stamp[row[i]] == j) return fail(QLDPC_EINVAL, "pos names a position twice");
            stamp[row[i]] = j;
        }
    }
    return QLDPC_OK;
}

int qldpc_select_positions_batch(qldpc_graph *g, const qldpc_rate_plan *plan, int32_t batch, const double *posterior,
                                 int32_t n_list, const int32_t *list, int32_t first, int32_t count, int32_t *pos,
                                 int32_t cap) {
    if (!g) return fail(QLDPC_EINVAL, "graph is NULL");
    if (batch < 0) return fail(QLDPC_EINVAL, "batch must be >= 0");
    int rc = check_window(batch, n_list, first, count, cap);
    if (rc) return rc;
    if (n_list == 0) return QLDPC_OK;
    if (!list || (count > 0 && (!posterior || !pos)) || (first > 0 && !pos)) return fail(QLDPC_EINVAL, "NULL host buffer");
    if ((rc = check_host_positions(g, plan, batch, n_list, list, pos, cap, first, count))) return rc;
    if ((rc = select_unsupported(count))) return rc;
    if ((rc = plan_on_every_device(g, plan))) return rc;
    if (g->devs.empty()) return fail(QLDPC_EINVAL, "a host-only graph cannot select on a device");
    if ((rc = select_fits(g, count))) return rc;
    if (count == 0) return QLDPC_OK;
    const size_t n = (size_t)g->n, w = (size_t)first + (size_t)count;  // the staged rows hold [0, first + count)
    return for_each_shard(
        g, n_list, "a host-only graph cannot select on a device",
        [&](DeviceGraph *dg, HostIO &io, int j0, int nb) -> int {
            const qldpc_rate_plan::Dev *pd = plan ? plan_dev(plan, dg->device) : nullptr;
            // only the listed frames' posterior rows and position histories travel
            std::vector<double> hpost((size_t)nb * n);
            std::vector<int32_t> hpos((size_t)nb * w, -1);
            for (int j = 0; j < nb; ++j) {
                const size_t f = (size_t)list[j0 + j];
                std::memcpy(hpost.data() + (size_t)j * n, posterior + f * n, n * sizeof(double));
                std::memcpy(hpos.data() + (size_t)j * w, pos + f * (size_t)cap, (size_t)first * sizeof(int32_t));
            }
            DevBuf<double> d_post;
            DevBuf<int32_t> d_pos;
            if (int r = d_post.alloc((size_t)nb * n)) return r;
            if (int r = d_pos.alloc((size_t)nb * w)) return r;
            auto enqueue = [&]() -> int {
                HIP_TRY(hipMemcpyAsync(d_post.get(), hpost.data(), hpost.size() * sizeof(double), hipMemcpyHostToDevice,
                                       io.stream));
                HIP_TRY(hipMemcpyAsync(d_pos.get(), hpos.data(), hpos.size() * sizeof(int32_t), hipMemcpyHostToDevice,
                                       io.stream));
                HIP_TRY(launch_select(g->n, nb, pd ? pd->cls.get() : nullptr, nb, nullptr, d_post.get(), first, count,
                                      d_pos.get(), (int)w, io.stream));
                HIP_TRY(hipMemcpyAsync(hpos.data(), d_pos.get(), hpos.size() * sizeof(int32_t), hipMemcpyDeviceToHost,
                                       io.stream));
                return QLDPC_OK;
            };
            const int r = enqueue();
            const hipError_t e = hipStreamSynchronize(io.stream);  // nothing of this call stays in flight
            if (r) return r;
            if (e != hipSuccess) return hip_fail(e, "select_positions_batch");
            for (int j = 0; j < nb; ++j)  // (distinct rows: the shards write disjoint frames)
                std::memcpy(pos + (size_t)list[j0 + j] * (size_t)cap + first, hpos.data() + (size_t)j * w + first,
                            (size_t)count * sizeof(int32_t));
            return QLDPC_OK;
        });
}

int qldpc_disclose_positions_batch(qldpc_graph *g, const qldpc_rate_plan *plan, int32_t batch, int32_t n_list,
                                   const int32_t *list, const uint8_t *ext, int64_t ext_stride, const int32_t *pos,
                                   int32_t cap, int32_t first, int32_t count, uint8_t *vals_out) {
    if (!g) return fail(QLDPC_EINVAL, "graph is NULL");
    if (batch < 0) return fail(QLDPC_EINVAL, "batch must be >= 0");
    int rc = check_window(batch, n_list, first, count, cap);
    if (rc) return rc;
    if (ext_stride < g->n) return fail(QLDPC_EINVAL, "ext_stride must be >= n");
    if (n_list == 0) return QLDPC_OK;
    if (!list || (count > 0 && (!ext || !pos || !vals_out))) return fail(QLDPC_EINVAL, "NULL host buffer");
    if ((rc = check_host_positions(g, plan, batch, n_list, list, pos, cap, count > 0 ? first + count : 0, -1))) return rc;
    if ((rc = plan_on_every_device(g, plan))) return rc;
    if (g->devs.empty()) return fail(QLDPC_EINVAL, "a host-only graph cannot disclose on a device");
    if (count == 0) return QLDPC_OK;
    const size_t n = (size_t)g->n, c = (size_t)count;
    return for_each_shard(
        g, n_list, "a host-only graph cannot disclose on a device",
        [&](DeviceGraph *, HostIO &io, int j0, int nb) -> int {
            // only the listed frames' rows and new positions travel
            std::vector<uint8_t> rows((size_t)nb * n);
            std::vector<int32_t> hpos((size_t)nb * c);
            for (int j = 0; j < nb; ++j) {
                const size_t f = (size_t)list[j0 + j];
                std::memcpy(rows.data() + (size_t)j * n, ext + f * (size_t)ext_stride, n);
                std::memcpy(hpos.data() + (size_t)j * c, pos + f * (size_t)cap + first, c * sizeof(int32_t));
            }
            DevBuf<uint8_t> d_rows, d_vals;
            DevBuf<int32_t> d_pos;
            if (int r = d_rows.alloc(rows.size())) return r;
            if (int r = d_vals.alloc((size_t)nb * c)) return r;
            if (int r = d_pos.alloc(hpos.size())) return r;
            auto enqueue = [&]() -> int {
                HIP_TRY(hipMemcpyAsync(d_rows.get(), rows.data(), rows.size(), hipMemcpyHostToDevice, io.stream));
                HIP_TRY(hipMemcpyAsync(d_pos.get(), hpos.data(), hpos.size() * sizeof(int32_t), hipMemcpyHostToDevice,
                                       io.stream));
                HIP_TRY(launch_disclose_positions(g->n, nb, nullptr, d_rows.get(), n, d_pos.get(), count, 0, count,
                                                  d_vals.get(), io.stream));
                HIP_TRY(hipMemcpyAsync(vals_out + (size_t)j0 * c, d_vals.get(), (size_t)nb * c, hipMemcpyDeviceToHost,
                                       io.stream));
                return QLDPC_OK;
            };
            const int r = enqueue();
            const hipError_t e = hipStreamSynchronize(io.stream);  // nothing of this call stays in flight
            if (r) return r;
            if (e != hipSuccess) return hip_fail(e, "disclose_positions_batch");
            return QLDPC_OK;
        });
}

int qldpc_reconcile_positions_round_batch(qldpc_graph *g, const qldpc_rate_plan *plan, const qldpc_params *p,
                                          int32_t batch, const uint8_t *key, const double *log_p,
                                          const uint8_t *syndrome, int32_t n_list, const int32_t *list,
                                          int32_t n_disc, const int32_t *pos, int32_t cap, const uint8_t *vals,
                                          uint8_t *bits_out, uint32_t *iters_out, uint8_t *synd_ok_out,
                                          double *posterior_out) {
    if (!g) return fail(QLDPC_EINVAL, "graph is NULL");
    int rc = check_params(p);
    if (rc) return rc;
    if (batch < 0) return fail(QLDPC_EINVAL, "batch must be >= 0");
    if ((rc = check_window(batch, n_list, 0, n_disc, cap))) return rc;
    if (n_list == 0) return QLDPC_OK;
    if (!key || !log_p || !syndrome || !list || !bits_out || !iters_out || !synd_ok_out ||
        (n_disc > 0 && (!pos || !vals)))
        return fail(QLDPC_EINVAL, "NULL host buffer");
    if ((rc = check_host_positions(g, plan, batch, n_list, list, pos, cap, n_disc, -1))) return rc;
    if ((rc = plan_on_every_device(g, plan))) return rc;
    if (g->devs.empty()) return fail(QLDPC_EINVAL, "a host-only graph cannot decode");
    if ((rc = positions_fit(g))) return rc;
    const size_t n = (size_t)g->n, m = (size_t)g->m, nd = (size_t)n_disc;
    return for_each_shard(
        g, n_list, "a host-only graph cannot decode", [&](DeviceGraph *dg, HostIO &io, int j0, int nb) -> int {
            if (int r = io.reserve((size_t)nb, n, m, false, true, true)) return r;
            const qldpc_rate_plan::Dev *pd = plan ? plan_dev(plan, dg->device) : nullptr;
            // only the listed frames' key rows, log_p, syndromes, positions and disclosed bytes travel
            std::vector<uint8_t> hkey((size_t)nb * n), hsynd((size_t)nb * m), hbits((size_t)nb * n), hok((size_t)nb);
            std::vector<double> hlogp((size_t)nb), hpost(posterior_out ? (size_t)nb * n : 0);
            std::vector<uint32_t> hiters((size_t)nb);
            std::vector<int32_t> hpos((size_t)nb * nd);
            for (int j = 0; j < nb; ++j) {
                const size_t f = (size_t)list[j0 + j];
                std::memcpy(hkey.data() + (size_t)j * n, key + f * n, n);
                std::memcpy(hsynd.data() + (size_t)j * m, syndrome + f * m, m);
                hlogp[j] = log_p[f];
                if (nd) std::memcpy(hpos.data() + (size_t)j * nd, pos + f * (size_t)cap, nd * sizeof(int32_t));
            }
            DevBuf<uint8_t> d_vals;
            DevBuf<int32_t> d_pos;
            if (int r = nd ? d_vals.alloc((size_t)nb * nd) : QLDPC_OK) return r;
            if (int r = nd ? d_pos.alloc(hpos.size()) : QLDPC_OK) return r;
            auto enqueue = [&]() -> int {
                HIP_TRY(hipMemcpyAsync(io.key.get(), hkey.data(), hkey.size(), hipMemcpyHostToDevice, io.stream));
                HIP_TRY(hipMemcpyAsync(io.logp.get(), hlogp.data(), nb * sizeof(double), hipMemcpyHostToDevice,
                                       io.stream));
                HIP_TRY(hipMemcpyAsync(io.synd.get(), hsynd.data(), hsynd.size(), hipMemcpyHostToDevice, io.stream));
                if (nd) {
                    HIP_TRY(hipMemcpyAsync(d_pos.get(), hpos.data(), hpos.size() * sizeof(int32_t),
                                           hipMemcpyHostToDevice, io.stream));
                    HIP_TRY(hipMemcpyAsync(d_vals.get(), vals + (size_t)j0 * nd, (size_t)nb * nd,
                                           hipMemcpyHostToDevice, io.stream));
                }
                if (int r = round_window(g, dg, pd, plan ? plan->n_punct : 0, p, nb, io.key.get(), io.logp.get(),
                                         io.synd.get(), nb, nullptr, n_disc, nullptr, d_vals.get(), io.bits.get(),
                                         io.iters.get(), io.ok.get(), posterior_out ? io.post.get() : nullptr,
                                         io.stream, true, d_pos.get(), n_disc))
                    return r;
                HIP_TRY(hipMemcpyAsync(hbits.data(), io.bits.get(), hbits.size(), hipMemcpyDeviceToHost, io.stream));
                HIP_TRY(hipMemcpyAsync(hiters.data(), io.iters.get(), nb * sizeof(uint32_t), hipMemcpyDeviceToHost,
                                       io.stream));
                HIP_TRY(hipMemcpyAsync(hok.data(), io.ok.get(), nb, hipMemcpyDeviceToHost, io.stream));
                if (posterior_out)
                    HIP_TRY(hipMemcpyAsync(hpost.data(), io.post.get(), hpost.size() * sizeof(double),
                                           hipMemcpyDeviceToHost, io.stream));
                return QLDPC_OK;
            };
            const int r = enqueue();
            const hipError_t e = hipStreamSynchronize(io.stream);  // nothing of this call stays in flight
            if (r) return r;
            if (e != hipSuccess) return hip_fail(e, "reconcile_positions_round_batch");
            if (int sc = split_check(g, dg, io.stream)) return sc;
            for (int j = 0; j < nb; ++j) {  // (distinct rows: the shards write disjoint frames)
                const size_t f = (size_t)list[j0 + j];
                std::memcpy(bits_out + f * n, hbits.data() + (size_t)j * n, n);
                iters_out[f] = hiters[j];
                synd_ok_out[f] = hok[j];
                if (posterior_out) std::memcpy(posterior_out + f * n, hpost.data() + (size_t)j * n, n * sizeof(double));
            }
            return QLDPC_OK;
        });
}

// ---- key verification and privacy amplification: the Toeplitz hash (privacy.hip) ----
// What both entries check before a device is touched; *done: batch == 0.
static int check_hash_args(int32_t batch, int32_t key_len, int64_t key_stride, const void *keys, int32_t out_len,
                           const void *seed, const int32_t *out_lens, bool host_lens, void *out, bool *done) {
    *done = false;
    if (batch < 0) return fail(QLDPC_EINVAL, "batch must be >= 0");
    if (key_len < 1 || out_len < 1) return fail(QLDPC_EINVAL, "key_len and out_len must be >= 1");
    if (key_stride < key_len) return fail(QLDPC_EINVAL, "key_stride must be >= key_len");
    if (batch == 0) {
        *done = true;
        return QLDPC_OK;
    }
    if (!keys || !seed || !out) return fail(QLDPC_EINVAL, host_lens ? "NULL host buffer" : "NULL device buffer");
    const size_t lds = toeplitz_hash_lds(key_len);
    if (lds > LDS_MAX_BYTES)
        return fail(QLDPC_EUNSUP, "key_len " + std::to_string(key_len) + ": the keys of a workgroup need " +
                                      std::to_string(lds) + " bytes of LDS (> " + std::to_string(LDS_MAX_BYTES) + ")");
    if (!toeplitz_hash_grid_ok(batch, out_len))
        return fail(QLDPC_EUNSUP, "batch x out_len is beyond one launch's grid");
    // (no buffer is read before this point; the device entry clamps in the kernel instead)
    if (host_lens && out_lens)
        for (int32_t f = 0; f < batch; ++f)
            if (out_lens[f] < 0 || out_lens[f] > out_len)
                return fail(QLDPC_EINVAL, "out_lens[" + std::to_string(f) + "] is outside [0, out_len]");
    return QLDPC_OK;
}

int qldpc_toeplitz_hash_device(int32_t batch, int32_t key_len, int64_t key_stride, const uint8_t *d_keys,
                               int32_t out_len, const uint8_t *d_seed, const int32_t *d_out_len, uint8_t *d_out,
                               void *stream) {
    bool done;
    if (int rc = check_hash_args(batch, key_len, key_stride, d_keys, out_len, d_seed, d_out_len, false, d_out, &done))
        return rc;
    if (done) return QLDPC_OK;
    const hipError_t e = launch_toeplitz_hash(batch, key_len, key_stride, d_keys, out_len, d_seed, d_out_len, d_out,
                                              (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "toeplitz_hash");
    return QLDPC_OK;
}

int qldpc_toeplitz_hash_batch(int32_t batch, int32_t key_len, int64_t key_stride, const uint8_t *keys,
                              int32_t out_len, const uint8_t *seed, const int32_t *out_lens, uint8_t *out) {
    bool done;
    if (int rc = check_hash_args(batch, key_len, key_stride, keys, out_len, seed, out_lens, true, out, &done))
        return rc;
    if (done) return QLDPC_OK;
    // staged on the current device for this call (the last row ends at its key_len)
    const size_t key_bytes = (size_t)(batch - 1) * (size_t)key_stride + (size_t)key_len;
    const size_t seed_bytes = (size_t)key_len + (size_t)out_len - 1, out_bytes = (size_t)batch * (size_t)out_len;
    DevBuf<uint8_t> d_keys, d_seed, d_out;
    DevBuf<int32_t> d_lens;
    int rc = d_keys.alloc(key_bytes);
    if (!rc) rc = d_seed.alloc(seed_bytes);
    if (!rc) rc = d_out.alloc(out_bytes);
    if (!rc && out_lens) rc = d_lens.alloc((size_t)batch);
    if (rc) {  // (any other failure, a missing device among them, keeps its own message)
        if (hipGetLastError() != hipErrorOutOfMemory) return rc;
        return fail(QLDPC_ENOMEM, "no device memory for " + std::to_string(key_bytes + seed_bytes + out_bytes) +
                                      " bytes of keys, seed and hash");
    }
    HIP_TRY(hipMemcpy(d_keys.get(), keys, key_bytes, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_seed.get(), seed, seed_bytes, hipMemcpyHostToDevice));
    if (out_lens) HIP_TRY(hipMemcpy(d_lens.get(), out_lens, (size_t)batch * sizeof(int32_t), hipMemcpyHostToDevice));
    const hipError_t e = launch_toeplitz_hash(batch, key_len, key_stride, d_keys.get(), out_len, d_seed.get(),
                                              out_lens ? d_lens.get() : nullptr, d_out.get(), nullptr);
    if (e != hipSuccess) return hip_fail(e, "toeplitz_hash");
    HIP_TRY(hipMemcpy(out, d_out.get(), out_bytes, hipMemcpyDeviceToHost));  // (after the kernel: the null stream)
    return QLDPC_OK;
}

// ---- the hash of one long block (privacy_block.hip) ----
int64_t qldpc_toeplitz_block_workspace(int64_t block_len, int64_t out_len) {
    if (block_len < 1 || out_len < 1) return fail(QLDPC_EINVAL, "block_len and out_len must be >= 1");
    const int k = toeplitz_block_log2(block_len, out_len);
    if (k < 0) return fail(QLDPC_EUNSUP, "block_len + out_len - 1 is beyond 2^27");
    return (int64_t)toeplitz_block_ws(k);
}

// What both entries check before a device is touched (the header's steps 1-5; the host entry brings
// a batch and no workspace); *done: n_list == 0.  *k_out: the transform's log2 size.
static int check_block_args(int32_t n_list, int32_t key_len, int64_t key_stride, const void *keys, int64_t out_len,
                            const void *seed, void *out, const void *ws, int64_t ws_bytes, bool host, int32_t batch,
                            bool *done, int *k_out) {
    *done = false;
    if (n_list < 0) return fail(QLDPC_EINVAL, "n_list must be >= 0");
    if (key_len < 1 || out_len < 1) return fail(QLDPC_EINVAL, "key_len and out_len must be >= 1");
    if (key_stride < key_len) return fail(QLDPC_EINVAL, "key_stride must be >= key_len");
    if (host && (batch < 0 || n_list > batch)) return fail(QLDPC_EINVAL, "batch must be >= 0 and n_list <= batch");
    if (n_list == 0) {
        *done = true;
        return QLDPC_OK;
    }
    if (!keys || !seed || !out || (!host && !ws))
        return fail(QLDPC_EINVAL, host ? "NULL host buffer" : "NULL device buffer");
    const int64_t L = (int64_t)n_list * key_len;
    const int k = toeplitz_block_log2(L, out_len);
    if (k < 0)
        return fail(QLDPC_EUNSUP, "block of " + std::to_string(L) + " bits and out_len " + std::to_string(out_len) +
                                      ": block + out_len - 1 is beyond 2^27");
    if (!host && ws_bytes < (int64_t)toeplitz_block_ws(k))
        return fail(QLDPC_EINVAL, "the workspace holds " + std::to_string(ws_bytes) + " bytes; " +
                                      std::to_string(toeplitz_block_ws(k)) + " are needed");
    *k_out = k;
    return QLDPC_OK;
}

int qldpc_toeplitz_hash_block_device(int32_t n_list, const int32_t *d_list, int32_t key_len, int64_t key_stride,
                                     const uint8_t *d_keys, int64_t out_len, const uint8_t *d_seed, uint8_t *d_out,
                                     void *d_ws, int64_t ws_bytes, void *stream) {
    bool done;
    int k;
    if (int rc = check_block_args(n_list, key_len, key_stride, d_keys, out_len, d_seed, d_out, d_ws, ws_bytes, false,
                                  0, &done, &k))
        return rc;
    if (done) return QLDPC_OK;
    const hipError_t e = launch_toeplitz_block(n_list, d_list, key_len, key_stride, d_keys, out_len, d_seed, d_out,
                                               d_ws, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "toeplitz_hash_block");
    return QLDPC_OK;
}

int qldpc_toeplitz_hash_block(int32_t batch, int32_t n_list, const int32_t *list, int32_t key_len, int64_t key_stride,
                              const uint8_t *keys, int64_t out_len, const uint8_t *seed, uint8_t *out) {
    bool done;
    int k;
    if (int rc = check_block_args(n_list, key_len, key_stride, keys, out_len, seed, out, nullptr, -1, true, batch,
                                  &done, &k))
        return rc;
    if (done) return QLDPC_OK;
    if (list)
        for (int32_t t = 0; t < n_list; ++t)
            if (list[t] < 0 || list[t] >= batch)
                return fail(QLDPC_EINVAL, "list[" + std::to_string(t) + "] is outside [0, batch)");
    // only the listed rows travel: the block is gathered here and staged on the current device
    const size_t kl = (size_t)key_len, L = (size_t)n_list * kl, seed_bytes = L + (size_t)out_len - 1;
    std::vector<uint8_t> block(L);
    for (int32_t t = 0; t < n_list; ++t)
        std::memcpy(block.data() + (size_t)t * kl, keys + (size_t)(list ? list[t] : t) * (size_t)key_stride, kl);
    DevBuf<uint8_t> d_block, d_seed, d_out, d_ws;
    int rc = d_block.alloc(L);
    if (!rc) rc = d_seed.alloc(seed_bytes);
    if (!rc) rc = d_out.alloc((size_t)out_len);
    if (!rc) rc = d_ws.alloc(toeplitz_block_ws(k));
    if (rc) {  // (any other failure, a missing device among them, keeps its own message)
        if (hipGetLastError() != hipErrorOutOfMemory) return rc;
        return fail(QLDPC_ENOMEM, "no device memory for " +
                                      std::to_string(L + seed_bytes + (size_t)out_len + toeplitz_block_ws(k)) +
                                      " bytes of block, seed, hash and workspace");
    }
    HIP_TRY(hipMemcpy(d_block.get(), block.data(), L, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_seed.get(), seed, seed_bytes, hipMemcpyHostToDevice));
    const hipError_t e = launch_toeplitz_block(n_list, nullptr, key_len, key_len, d_block.get(), out_len, d_seed.get(),
                                               d_out.get(), d_ws.get(), nullptr);
    if (e != hipSuccess) return hip_fail(e, "toeplitz_hash_block");
    HIP_TRY(hipMemcpy(out, d_out.get(), (size_t)out_len, hipMemcpyDeviceToHost));  // (after the kernels: the null stream)
    return QLDPC_OK;
}

// ---- trial generator (src/simulation.cpp:540-551,713-719,743) ----------------
int qldpc_xoshiro_jump(uint64_t seed, uint64_t draws, uint64_t *state_out) {
    if (!state_out) return fail(QLDPC_EINVAL, "NULL state_out");
    return xoshiro_jump_check(seed, draws, state_out);
}

int qldpc_trials_device(int32_t n, double qber, int32_t batch, const uint64_t *d_seeds, uint64_t seed_add,
                        uint8_t *d_alice, uint8_t *d_bob, double *accurate_qber_out, void *stream) {
    if (n <= 0 || batch < 0) return fail(QLDPC_EINVAL, "n must be > 0 and batch >= 0");
    const uint64_t n_err = (uint64_t)((double)n * qber);
    if (n_err == 0)  // run_trial's own check (src/simulation.cpp:552-553)
        return fail(QLDPC_EINVAL, "Key size '" + std::to_string(n) + "' is too small for QBER.");
    if (n_err > (uint64_t)n) return fail(QLDPC_EINVAL, "QBER must be <= 1");
    if (accurate_qber_out) *accurate_qber_out = (double)n_err / (double)n;
    if (batch == 0) return QLDPC_OK;
    if (!d_seeds || !d_alice || !d_bob) return fail(QLDPC_EINVAL, "NULL device buffer");
    const hipStream_t s = (hipStream_t)stream;
    uint32_t *scratch = nullptr;
    HIP_TRY(trial_workspace(s, trials_scratch_words(n, n_err, 0, batch), &scratch));
    hipError_t e = launch_trials(n, n_err, batch, d_seeds, seed_add, d_alice, d_bob, scratch, 0, nullptr, nullptr, s);
    if (e != hipSuccess) return hip_fail(e, "trials");
    return QLDPC_OK;
}

}  // extern "C"
