// graph.hpp — what the host files of libqkdldpc_hip.so share: the graph and its
// per-device state, the error helpers, the types that own device memory,
// pinned memory, events, streams and the current device, and the few functions
// that cross files (plan.hip, layout.hip, capi.hip, run_trials.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/qkd_ldpc_hip.h"
#include "decoder.hpp"

namespace qldpc {

extern thread_local std::string g_last_error;  // capi.hip (qldpc_last_error)
int fail(int code, const std::string &msg);
int hip_fail(hipError_t e, const char *what);

#define HIP_TRY(expr)                                         \
    do {                                                      \
        hipError_t _e = (expr);                               \
        if (_e != hipSuccess) return hip_fail(_e, #expr);     \
    } while (0)

constexpr size_t LDS_LIMIT = 160 * 1024;
// DecodeArgs::exit_gate of every launch (capi.hip exit_gate(); the SPA register
// decoder's parity-only pass, decoder_v2.hip).  The smallest count that
// precedes >= 99 % of the exits of C2's converging frames, measured with the
// oracle on the bench's own trials (tools/exit_gate_stats.py, DESIGN.md §3.3:
// 1024 C2 frames want 54, 4096 C1 frames 36 — a constant serves both).
constexpr int V2_EXIT_GATE = 54;

// ---- owners (move-only) -------------------------------------------------------
// Device memory (hipMalloc / hipFree) or, Pinned, host memory the copies stay
// asynchronous with (hipHostMalloc / hipHostFree).
template <typename T, bool Pinned>
class GpuBuf {
    T *p_ = nullptr;
    static hipError_t release(T *p) { return Pinned ? hipHostFree(p) : hipFree(p); }

public:
    GpuBuf() = default;
    GpuBuf(const GpuBuf &) = delete;
    GpuBuf &operator=(const GpuBuf &) = delete;
    GpuBuf(GpuBuf &&o) noexcept : p_(o.p_) { o.p_ = nullptr; }
    GpuBuf &operator=(GpuBuf &&o) noexcept {
        std::swap(p_, o.p_);
        return *this;
    }
    ~GpuBuf() {
        if (p_) (void)release(p_);
    }
    T *get() const { return p_; }
    explicit operator bool() const { return p_ != nullptr; }
    // Free, then allocate max(count, 1) elements.  (The caller synchronises
    // first when the old buffer may still be in use.)
    int alloc(size_t count) {
        if (p_) HIP_TRY(release(p_));
        p_ = nullptr;
        const size_t bytes = std::max<size_t>(count, 1) * sizeof(T);
        if (Pinned) HIP_TRY(hipHostMalloc(&p_, bytes));
        else HIP_TRY(hipMalloc(&p_, bytes));
        return QLDPC_OK;
    }
    int upload(const std::vector<T> &src) {
        static_assert(!Pinned, "upload is for device buffers");
        if (int rc = alloc(src.size())) return rc;
        if (!src.empty()) HIP_TRY(hipMemcpy(p_, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
        return QLDPC_OK;
    }
};
template <typename T>
using DevBuf = GpuBuf<T, false>;
template <typename T>
using PinnedBuf = GpuBuf<T, true>;

// An event or stream its holder created (`if (!h) HIP_TRY(hipEventCreate(h.put()))`).
template <typename H, hipError_t (*Destroy)(H)>
class Owned {
    H h_ = nullptr;

public:
    Owned() = default;
    Owned(const Owned &) = delete;
    Owned &operator=(const Owned &) = delete;
    Owned(Owned &&o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    Owned &operator=(Owned &&o) noexcept {
        std::swap(h_, o.h_);
        return *this;
    }
    ~Owned() {
        if (h_) (void)Destroy(h_);
    }
    H get() const { return h_; }
    operator H() const { return h_; }
    H *put() { return &h_; }
};
using Event = Owned<hipEvent_t, hipEventDestroy>;
using Stream = Owned<hipStream_t, hipStreamDestroy>;

// The caller's current device, restored when the scope ends.
class DeviceScope {
    int prev_ = -1;

public:
    DeviceScope() = default;
    DeviceScope(const DeviceScope &) = delete;
    DeviceScope &operator=(const DeviceScope &) = delete;
    ~DeviceScope() {
        if (prev_ >= 0) (void)hipSetDevice(prev_);
    }
    int save() {  // (the devices are then selected by the work itself)
        int d = 0;
        HIP_TRY(hipGetDevice(&d));
        prev_ = d;
        return QLDPC_OK;
    }
    int enter(int device) {
        if (int rc = save()) return rc;
        HIP_TRY(hipSetDevice(device));
        return QLDPC_OK;
    }
};

// ---- per-device state ---------------------------------------------------------
struct Workspace {  // per (device, stream): frame counter + decoder scratch
    DevBuf<int> counter;
    DevBuf<double> scratch;
    size_t scratch_doubles = 0;
    // V2 frame format (palette + 2-bit codes), capacity in frames
    DevBuf<uint8_t> codes, pal_ok;
    DevBuf<double> palette;
    size_t code_frames = 0;
    // V2 split frames: group claim / publish / barrier / mismatch slots and the
    // frames' totals, capacity in frames
    DevBuf<int> split_ctl;
    DevBuf<double> gtotal, gstage;
    size_t split_frames = 0;
    // frame claim order (order.hip): per-frame weights and the sorted order
    DevBuf<int32_t> fweight, forder;
    size_t order_frames = 0;
    int order_count = 0;  // frames of the last decode claimed through forder (0: index order)
    // the fused entries' frame LLRs when the caller passes no workspace and the
    // graph's decoder reads llr[] (not V2), capacity in frames
    DevBuf<double> llr_ws;
    size_t llr_ws_frames = 0;
    // a disclosure round's compact frames (qldpc_reconcile_round_device): the
    // pinned LLRs and syndromes the decoder reads, and its results before the
    // scatter, capacity in frames; the posteriors only once a caller asks
    DevBuf<double> round_llr, round_post;
    DevBuf<uint8_t> round_synd, round_bits, round_ok;
    DevBuf<uint32_t> round_iters;
    size_t round_frames = 0, round_post_frames = 0;
    // frame-per-lane tiles (decoder_fpl.hip): messages, totals, LLRs and lane
    // masks of one chunk, capacity in tiles
    DevBuf<uint64_t> fpl;
    size_t fpl_tiles = 0;
    // ... and of a traced decode: 64 per-lane counters per tile (FplTrace::cnt), capacity in tiles
    DevBuf<uint32_t> fpl_trace_cnt;
    size_t fpl_trace_tiles = 0;
    // the syndrome weights of an estimate whose caller takes only q / log_p, capacity in frames
    DevBuf<int32_t> est_weight;
    size_t est_frames = 0;
    // kernel timing (qldpc_set_kernel_timing): events around the last decode launch
    Event ev0, ev1;
    bool ev_recorded = false;
};

struct HostIO {  // device staging buffers of the host-buffer entries
    DevBuf<double> llr, post;
    DevBuf<uint8_t> synd, bits, ok;
    DevBuf<uint32_t> iters;
    // the per-party entries' inputs: a party's key bytes and Bob's log_p
    DevBuf<uint8_t> key;
    DevBuf<double> logp;
    // capacities in frames, one per group an entry may do without: the LLRs
    // (qldpc_decode_batch alone), the decode results, the syndromes, the keys
    size_t cap_frames = 0, cap_out = 0, cap_synd = 0, cap_key = 0;
    Stream stream;
    // Grow the groups a call stages (the caller holds io_mu; nothing of an
    // earlier call is in flight: each entry ends with a stream sync).
    int reserve(size_t nb, size_t n, size_t m, bool want_llr, bool want_out, bool want_key) {
        int r;
        if (want_llr && nb > cap_frames) {
            cap_frames = 0;
            if ((r = llr.alloc(nb * n))) return r;
            cap_frames = nb;
        }
        if (want_out && nb > cap_out) {
            cap_out = 0;
            if ((r = post.alloc(nb * n)) || (r = bits.alloc(nb * n)) || (r = ok.alloc(nb)) || (r = iters.alloc(nb)))
                return r;
            cap_out = nb;
        }
        if (nb > cap_synd) {
            cap_synd = 0;
            if ((r = synd.alloc(nb * m))) return r;
            cap_synd = nb;
        }
        if (want_key && nb > cap_key) {
            cap_key = 0;
            if ((r = key.alloc(nb * n)) || (r = logp.alloc(nb))) return r;
            cap_key = nb;
        }
        return QLDPC_OK;
    }
};

// qldpc_run_trials: one pipeline slot of a device's trial batches — the
// chunk's seeds, keys and results on device, its results in pinned host memory
// (two slots per device: chunk c + 1's trials are generated while chunk c
// decodes on the other stream).
struct TrialSlot {
    Stream stream;
    // the chunk's window: from ev0 (after its trials are generated) or the end
    // of the other slot's chunk before it (prev_end), whichever is later, to
    // ev1 (after the key compare).  ev1 alternates over ev_end, so the other
    // slot's next chunk never re-records the end a window is measured from.
    // (ev1 and prev_end alias an ev_end of this or the other slot: not owned.)
    Event ev0, ev_end[2];
    hipEvent_t ev1 = nullptr, prev_end = nullptr;
    int ev_i = 0;
    DevBuf<uint64_t> seeds, clk;
    DevBuf<uint8_t> alice, bob, palice, pbob, alice_ext;
    DevBuf<uint8_t> synd, bits, ok, km;
    DevBuf<uint32_t> iters, tscratch;
    DevBuf<double> logp;
    PinnedBuf<uint32_t> h_iters;
    PinnedBuf<uint8_t> h_ok, h_km;
    PinnedBuf<uint64_t> h_clk, h_seeds;  // pinned: the copies stay asynchronous
    PinnedBuf<double> h_logp;
    size_t cap = 0, cap_punct = 0, tscratch_words = 0;
    int f0 = 0, nb = 0;  // the chunk in flight (nb == 0: none)
    qldpc_trials_job *owner = nullptr;  // the job whose results it holds
};

// ---- the graph's index tables ---------------------------------------------------
// Every table layout.hip builds from H, once: X(element type, name, when it
// exists on a device, whether layout_digest hashes it).  GraphTables (the host
// vectors), DeviceGraph's table members, upload_tables (capi.hip) and
// layout_digest (layout.hip) are generated from this list, in this order (line
// by line, left to right): the upload's, and the digest's that
// tests/test_layout.py pins.  A table that does not exist on a device stays a
// NULL pointer there, which the launches test; a T_ALWAYS table is allocated
// even when it is empty.  T_FPL: frame-per-lane graphs (VAR_FPL); T_PAIRED:
// g.paired, the v1 occurrence pairing of an unsorted adjacency; T_RELABELLED:
// V2 bank relabelling (col_orig non-empty).
enum TableWhen { T_ALWAYS, T_FPL, T_PAIRED, T_RELABELLED, T_WHEN_COUNT };
#define QLDPC_GRAPH_TABLES(X)                                                                                          \
    X(uint32_t, slot_meta, T_ALWAYS, true) X(uint32_t, slot_meta_ms, T_ALWAYS, true) /* _ms: min-sum, rows by kpos */  \
    X(uint64_t, vn_mask, T_ALWAYS, true) X(uint64_t, vn_mask_ms, T_ALWAYS, true) /* V2: [wave][dv_max] slot masks */   \
    X(uint64_t, vn_exec, T_ALWAYS, true) X(uint64_t, vn_exec_ms, T_ALWAYS, true) /* V2: [wave][dv_max][slot] lanes */  \
    X(uint32_t, slot_meta2, T_ALWAYS, true) X(uint32_t, slot_meta2_ms, T_ALWAYS, true) /* hybrid: slot's stage pos */   \
    X(int32_t, hd_bits, T_ALWAYS, true) X(int32_t, hd_dv, T_ALWAYS, true) X(int32_t, stage_off, T_ALWAYS, true)        \
    X(int32_t, row_orig, T_ALWAYS, true)  /* V2: layout row -> original row (syndrome index) */                        \
    X(int32_t, part_row0, T_ALWAYS, true) /* V2 split: first layout row of each part */                                \
    X(int32_t, xoff, T_ALWAYS, true)      /* V2 split exchange: region starts */                                       \
    X(uint16_t, xbit, T_ALWAYS, true) X(uint16_t, xbit_ms, T_ALWAYS, true) /* ... stage position's chunk-local bit */  \
    X(int32_t, lane_row0, T_ALWAYS, true) X(int32_t, wave_rows, T_ALWAYS, true) X(int32_t, lane_head, T_ALWAYS, true)  \
    X(int32_t, lane_nst, T_ALWAYS, true) X(int32_t, lane_epl, T_ALWAYS, true) X(int32_t, ell_col, T_ALWAYS, true)      \
    X(int32_t, row_deg, T_ALWAYS, true) X(int32_t, iso_bits, T_ALWAYS, true)                                           \
    X(uint32_t, vn_rows, T_ALWAYS, true) /* V2 min-sum bit gather: [n or chunks][2] four u16 layout rows */            \
    X(uint32_t, vng_bits, T_ALWAYS, true) X(uint32_t, vng_meta2, T_ALWAYS, true) /* hybrid bit gather: order, slots */ \
    X(uint64_t, row_sem, T_ALWAYS, true)   /* V2 scan: [wave][slot][4] START / END / PARK lane masks (+ pad) */        \
    X(uint32_t, vng_rec, T_ALWAYS, true)   /* register-shape bit gather: per slot, byte offset | shift << 16 */        \
    X(uint64_t, row_rmask, T_ALWAYS, true) /* V2 scan: [row j][lane] slots of the lane's j-th started row */           \
    X(int32_t, fpl_row_ptr, T_FPL, false) X(int32_t, fpl_col, T_FPL, false) /* frame-per-lane: CSR */                  \
    X(int32_t, fpl_cslot, T_FPL, false) X(int32_t, fpl_col_ptr, T_FPL, false) /* ... edge's bit_nodes slot, CSC starts */ \
    X(int32_t, fpl_rows, T_FPL, false)    /* ... rows by length class */                                               \
    X(int32_t, pair_src, T_PAIRED, true) X(int32_t, pair_col, T_PAIRED, true) /* [k][lane] */                          \
    X(int32_t, col_orig, T_RELABELLED, true) X(int32_t, col_lab, T_RELABELLED, true) /* label -> bit id and back */    \
    X(int32_t, ell_lab, T_RELABELLED, true) /* row-ELL in labels (the claim order reads label-ordered frame codes) */

struct DeviceGraph {
    int device = 0;
    int num_cus = 0;
#define QLDPC_X(type, name, when, digested) DevBuf<type> name;
    QLDPC_GRAPH_TABLES(QLDPC_X)
#undef QLDPC_X
    std::mutex mu;     // workspaces (ws), occupancy cache
    std::map<void *, Workspace> ws;
    std::mutex io_mu;  // the host-buffer entry's staging buffers and stream, held copy-in .. copy-out
    HostIO io;
    std::mutex trial_mu;  // qldpc_run_trials' pipeline slots: held while a job enqueues or harvests
    TrialSlot tslot[2];
    int next_slot = 0;    // the slot the next chunk takes (the two alternate)
    int occ[6] = {0, 0, 0, 0, 0, 0};
    DeviceGraph() = default;
    // Its device is selected (the caller restores its own) and idle before the
    // members release what they own.
    ~DeviceGraph() {
        (void)hipSetDevice(device);
        (void)hipDeviceSynchronize();
    }
};

// The index tables of one graph on the host: one vector per entry of
// QLDPC_GRAPH_TABLES, under the entry's name (layout.hip fills them, capi.hip
// uploads them to each device).
struct GraphTables {
#define QLDPC_X(type, name, when, digested) std::vector<type> name;
    QLDPC_GRAPH_TABLES(QLDPC_X)
#undef QLDPC_X
    bool relabelled() const { return !col_orig.empty(); }  // T_RELABELLED
};

}  // namespace qldpc

namespace qldpc {
// Error estimation (capi.hip est_row_table): per check row its effective degree
// when it is informative — no punctured neighbour, at least one neighbour that
// is not shortened — else 0, and the classes of the informative rows: the
// distinct effective degrees, ascending, with their row counts.
struct EstTable {
    std::vector<int32_t> row_d, degree, rows;
    int64_t informative = 0;  // R, the sum of rows[]
};
}  // namespace qldpc

// Rate-adaptation plan: per position its class (0 key, 1 punctured, 2
// shortened) and source index, replicated on the graph's devices; the class
// bytes on the host too, and the estimator's row table of the graph the plan
// was created for (adjacency: that graph's qldpc_graph::adjacency).
struct qldpc_rate_plan {
    struct Dev {
        int device;
        qldpc::DevBuf<uint8_t> cls;
        qldpc::DevBuf<int32_t> src;
        qldpc::DevBuf<int32_t> row_d;
    };
    int n_punct = 0, n_short = 0;
    std::vector<uint8_t> cls;
    qldpc::EstTable est;
    uint64_t adjacency = 0;
    std::vector<Dev> devs;
};

struct qldpc_graph {
    int n = 0, m = 0, E = 0, T = 0, EPL = 0, dv_max = 0, max_dc = 0, variant = 0;
    bool vng = false;                       // V2 min-sum bit gather tables built
    bool vng_h_fit = false;                 // hybrid bit gather's padded edge codes fit LDS (set before planning)
    bool rows_global_ms = false;            // hybrid min-sum: row aggregates (partly) in global scratch
    int rows_lds_ms = 0, rows_lds_waves_ms = 0;  // ... of which the rows of the first waves stay in LDS
    int v2R = 0, v2RG = 0, n_iso = 0;       // V2: register / scratch slots per lane, bits of degree 0
    std::vector<int> wave_rows;             // V2: first layout row of each wave (+ m)
    std::vector<int> row_order;             // V2: layout row -> original row
    std::vector<int> layout_row_ptr;        // V2: row_ptr of the rows in layout order
    int vn_k0 = 0, n_hd = 0;                // V2 hybrid: first staged VN term, bits of degree > vn_k0
    bool paired = false;                    // unsorted adjacency: v1 global-slot kernel with occurrence pairing
    int hd_uniform_dv = 0;                  // > 0: the staged bits are 0..n-1 in order, all of this degree
    int nst_max = 0;                        // V2 SPA scan: most rows started in one lane (row_rmask rows)
    long long stage_doubles = 0;            // V2 hybrid: staged VN terms per frame
    int split_k = 1, split_mrows = 0;       // V2 split: workgroups per frame, rows of the largest part
    int split_cb = 0, split_nc = 0;         // V2 split exchange gather: bits per LDS chunk, chunks per part (0: off)
    int split_pl = qldpc::REG_TSTRIDE;      // V2 split: a part's lanes (1024: 16 waves; 512: 8 waves, 2 per CU)
    bool kernel_timing = false;             // qldpc_set_kernel_timing
    std::vector<int32_t> col_lab;           // V2 bank relabelling (relabel.cpp): bit id -> label; empty: identity
    long long relabel_stats[4] = {0, 0, 0, 0};  // bank excess before / after, busiest-bank cycles before / after
    std::vector<int> part_row0;             // V2 split: first layout row of each part (+ m)
    int fpl_class_off[qldpc::FPL_CLASSES + 1] = {};  // frame-per-lane: rows by length class (GraphTables::fpl_rows)
    // error estimation: the row-ELL adjacency on the host (GraphTables::ell_col /
    // row_deg), a hash of it (a plan's row table belongs to one adjacency) and
    // the row table without a plan (row_d is row_deg itself there: left empty)
    std::vector<int32_t> h_ell_col, h_row_deg;
    uint64_t adjacency = 0;
    qldpc::EstTable est;
    std::vector<std::unique_ptr<qldpc::DeviceGraph>> devs;
};

namespace qldpc {

// plan.hip — (variant, T, EPL) and the V2 row deal of a classified graph
int env_int(const char *name, int dflt);  // a QLDPC_* knob under the diagnostic switch
void plan(qldpc_graph &g);
bool plan_v2(qldpc_graph &g, const int32_t *row_ptr);
bool plan_v2_split(qldpc_graph &g, const int32_t *row_ptr, const int32_t *col_idx);
// ... and what a decode of the planned graph launches (every variant; V2 through
// decoder_v2.hip's v2_launch_shape).  vng_enabled: the QLDPC_VNG knob, as vng_enabled() reads it.
bool vng_enabled();
LaunchShape launch_shape(const qldpc_graph &g, int alg, bool vng_enabled);
void print_launch_shapes(const qldpc_graph &g);  // the {"launch": ...} lines of QLDPC_DEBUG_PLAN

// layout.hip — validate, plan, build every table; touches no device.  layout:
// QLDPC_LAYOUT_AUTO (the planner's choice) or QLDPC_LAYOUT_FRAME_PER_LANE.
int build_layout(int32_t n, int32_t m, const int32_t *row_ptr, const int32_t *col_idx, const int32_t *col_ptr,
                 const int32_t *row_idx, std::unique_ptr<qldpc_graph> &out, GraphTables &t,
                 int layout = QLDPC_LAYOUT_AUTO);

// capi.hip — used by run_trials.hip
int check_params(const qldpc_params *p);
int split_check(qldpc_graph *g, DeviceGraph *dg, hipStream_t stream);
int qkd_ldpc_window(qldpc_graph *g, DeviceGraph *dg, const qldpc_rate_plan *plan, const qldpc_params *p, int batch,
                    const uint8_t *d_alice, const uint8_t *d_bob, const uint8_t *d_punct_alice,
                    const uint8_t *d_punct_bob, const double *d_log_p, uint8_t *d_alice_ext, double *d_llr_ws,
                    uint8_t *d_synd_ws, uint8_t *d_bits_out, uint32_t *d_iters_out, uint8_t *d_synd_ok_out,
                    uint8_t *d_keys_match_out, hipStream_t s, uint64_t *frame_clk = nullptr,
                    hipEvent_t before_decode = nullptr);

}  // namespace qldpc
