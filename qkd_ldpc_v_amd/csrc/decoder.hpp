// decoder.hpp — host/device shared definitions of the gfx950 LDPC decoder.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

namespace qldpc {

// Per-slot metadata word (slot-major [slot][lane], one uint32 per CSR edge).
constexpr uint32_t META_COL_MASK = 0xFFFFFu;   // bit id (n <= 2^20)
constexpr int META_KPOS_SHIFT = 20;            // position of the edge in its bit's check list
constexpr uint32_t META_KPOS_MASK = 0x1FFu;    // dv < 511 (511 marks a V2 dummy slot)
constexpr uint32_t META_START = 1u << 29;      // first edge of its row
constexpr uint32_t META_END = 1u << 30;        // last edge of its row
constexpr uint32_t META_VALID = 1u << 31;      // slot holds an edge (tail padding otherwise)
constexpr int MAX_DV = (int)META_KPOS_MASK;
constexpr int MAX_N = 1 << 20;

// Registers available for per-edge messages in the register-resident variant.
constexpr int EPL_REG = 40;
// Lane stride of the register variant's metadata groups (== max lanes).
constexpr int REG_TSTRIDE = 1024;

enum Variant : int {
    VAR_REG_LDS = 0,  // messages in VGPRs, totals/rows in LDS       (n <~ 14k)
    VAR_GLB_LDS = 1,  // messages in per-workgroup global scratch, totals/rows in LDS
    VAR_GLB_GLB = 2,  // everything per-frame in global scratch     (n = 100k)
    VAR_V2 = 3,       // wave-aligned register kernel (decoder_v2.hip)
    VAR_FPL = 4,      // frame-per-lane: 64 frames per wave, a launch sequence per iteration (decoder_fpl.hip)
};

// Register slots per lane of the V2 instantiations.  (A third, 84 slots x 8
// waves, holds no more edges than 56 x 12 and its SPA build falls back to a
// scratch array, so it is not built.)
constexpr int V2_R_TIGHT = 40, V2_R_SMALL = 44, V2_R_MID = 56;
#ifndef QL_SPLIT_R
#define QL_SPLIT_R 40  // split frames' slots per lane (A/B: 44, 48 with a matching capi build)
#endif
constexpr int V2_R_SPLIT = QL_SPLIT_R;
// Split frames may add this many message slots per lane in per-workgroup
// global scratch to the V2_R_SPLIT register/LDS slots (round 6): more edges
// per part, so fewer parts per frame and more frames per XCD.  The planner
// takes them only when they raise frames per XCD by >= 4/3 (plan.hip
// plan_v2_split).
#ifndef QL_SPLIT_RG
#define QL_SPLIT_RG 12
#endif
constexpr int V2_RG_SPLIT = QL_SPLIT_RG;
static_assert(V2_RG_SPLIT > 0 && V2_RG_SPLIT % 4 == 0 && V2_R_SPLIT + V2_RG_SPLIT <= 64,
              "split scratch slots: groups of four, <= 64 slots in all");
constexpr int V2_CODES_CAP = 20480;  // V2: bits per frame whose palette indices fit LDS (n <= this)
// Hybrid instantiation: 44 VGPR slots + this many slots in per-workgroup global scratch.
constexpr int V2_RG_HYBRID = 20;
// SPA-family register kernels at V2_R_TIGHT keep this many message slots in LDS
// (when the frame's LDS image leaves room) instead of VGPRs.  5: the C2 image
// is then 159.8 KiB, and the kernel spills fewer VGPRs to scratch than with 4
// (same-box A/B: 0.6% faster decode, profiles/r04/ab_rl5.txt).
#ifndef QL_RL
#define QL_RL 5
#endif
constexpr int V2_RL = QL_RL;
// Workgroup size each V2 instantiation is compiled for (its VGPR budget).
constexpr __host__ __device__ int v2_threads_for(int R) { return R <= V2_R_SMALL ? 1024 : 768; }

// Phase ids of the diagnostic stamp build (QL_PHASE_STAMPS).
enum StampId : int {
    ST_SETUP, ST_SETUP_WAIT, ST_S, ST_S_WAIT, ST_CN1, ST_CN1_WAIT, ST_CN2, ST_CN2_WAIT, ST_CN3,
    ST_VN0, ST_VN0_WAIT, ST_VNK, ST_VNK_WAIT, ST_OUT, ST_OUT_WAIT,
    ST_GATE,  // the SPA exit gate's parity-only pass and its barrier wait
    NUM_STAMPS
};
static const char *const STAMP_NAMES[NUM_STAMPS] = {
    "setup", "setup_wait", "synd", "synd_wait", "cn1", "cn1_wait", "cn2", "cn2_wait", "cn3",
    "vn_init", "vn_init_wait", "vn_phases", "vn_phases_wait", "out", "out_wait", "exit_pass"};

struct DecodeArgs {
    // graph (device pointers; shared by every frame)
    int n, m, E, T, EPL, dv_max, max_dc;
    const uint32_t *slot_meta;  // [ceil(EPL/4)][T][4]: uint4 per 4 slots
    const int32_t *lane_row0;   // [T] row of slot 0 (or -1)
    const int32_t *lane_head;   // [T] leading slots that finish a row begun in lane-1
    const int32_t *lane_nst;    // [T] V2: rows started in the lane
    const int32_t *lane_epl;    // [T] V2: slots of the lane's wave (uniform per wave)
    const int32_t *ell_col;     // [max_dc][m] bit ids of each row, row-ELL, slot-major
    const int32_t *row_deg;     // [m]
    // decoder parameters
    int alg, max_it, thr_on;
    double thr, primary, secondary;
    // SPA edge-form constants, computed by the host C library (capi.hip fill_args):
    double spa_tlim;  // tanh(min(thr, 44) / 2.)  (1 when clipping is off)
    double spa_ctop;  // 2. * atanh(1 - 2^-53)
    // frames
    int batch;
    const double *llr;      // [batch][n]
    const uint8_t *synd;    // [batch][m]
    uint8_t *bits;          // [batch][n]
    uint32_t *iters;        // [batch]
    uint8_t *ok;            // [batch]
    double *post;           // [batch][n] or nullptr
    // scheduling / scratch
    int *frame_counter;
    const int32_t *frame_order;   // [batch] claim order (order.hip); nullptr: index order
    double *scratch;              // per-workgroup scratch (variants 1, 2)
    long long scratch_wg_doubles; // doubles per workgroup
    uint64_t *stamps;             // diagnostic build only: [wg][wave][NUM_STAMPS]
    // V2 frame format: channel LLRs as a 4-entry palette + 2-bit codes
    int nc;                  // code bytes per frame = ceil(n / 4)
    const uint8_t *codes;    // [batch][nc]
    const double *palette;   // [batch][4]
    const uint8_t *pal_ok;   // [batch]; 0 -> the decoder gathers llr[] instead
    int n_iso;               // bits with no check (dv = 0): total = llr
    const int32_t *iso_bits; // [n_iso]
    int v2R;                 // register slots of the V2 instantiation to launch
    int v2RG;                // + slots in per-workgroup global scratch (0 or V2_RG_HYBRID)
    const uint64_t *vn_mask; // [waves][dv_max]: slots holding a kk-th bit edge, per wave
    const uint64_t *vn_exec; // [waves][dv_max][slots]: lanes whose slot holds a kk-th bit edge
    // V2 hybrid: VN terms k >= vn_k0 are staged in scratch by the message pass
    // and summed per bit in one gather pass (bits sorted by degree, descending).
    int vn_k0;                      // first staged term (dv_max: none)
    int n_hd;                       // bits with degree > vn_k0
    const int32_t *hd_bits;         // [n_hd]
    const int32_t *hd_dv;           // [n_hd]
    int hd_uniform_dv;              // > 0: hd_bits[i] == i and hd_dv[i] == this for every i
    const int32_t *stage_off;       // [dv_max]: offset of term kk's block in the stage
    const uint32_t *slot_meta2;     // like slot_meta: stage index of the slot's edge
    long long stage_wg_offset;      // doubles from a workgroup's scratch base to its stage
    const int32_t *row_orig;        // V2: layout row -> original row (syndrome index)
    // V2 scan (one workgroup per frame, register slots only): the row
    // structure as lane masks and per-lane row slot masks (layout.hip build_meta)
    const uint64_t *row_sem;        // [waves][slots][4]: the lanes whose slot starts / ends a row / parks a tail
    const uint64_t *row_rmask;      // [nst_max][T]: slots of the lane's j-th started row; bit 63: open
    int nst_max;
    // V2 split frames (split_k > 1 workgroups of one XCD per frame)
    int split_k;                    // parts per frame (1: not split)
    int split_mrows;                // rows of the largest part (LDS rows array)
    int split_slots;                // group slots per XCD in the arrays below
    const int32_t *part_row0;       // [split_k + 1] first layout row of each part
    int *split_claim;               // [16] per-XCD claim counters
    int *split_pub;                 // [16][slots] frame + 1, published by rank 0
    int *split_sync;                // [16][slots] group barrier arrivals
    int *split_mis;                 // [16][slots] iteration + 1 of the last row mismatch
    double *gtotal;                 // [batch][n + 1] the frames' totals
    int *split_err;                 // set when a part group failed to meet (results void)
    double *gstage;                 // [batch][stage_frame_doubles] split frames' VN stage
    long long stage_frame_doubles;
    // Split-frame exchange layout (nullptr xoff: the term-major stage).  Part p
    // owns bits [n p / K, n (p + 1) / K) in split_nc chunks of split_cb; the
    // stage is one region per (owner part, chunk, kpos), each holding its terms
    // in (writer wave, slot, lane) order, so a writing wave fills whole lines
    // and the owner reads each region front to back, adding every term into
    // an LDS sum at the bit's chunk-local index xbit[position].
    int split_cb, split_nc;
    const int32_t *xoff;            // [K * nc * dv_max + 1] region starts (doubles into the frame's stage)
    const uint16_t *xbit;           // [stage_frame_doubles] chunk-local bit of each stage position
    // v1 global-slot kernels, unsorted adjacency (occurrence pairing): input
    // slot s of the next check-node pass gets total[pair_col[s]] -
    // c2b[pair_src[s]] (both [k][lane]); the values go through a slot-major
    // buffer at pair_buf_off doubles into the workgroup's scratch.  nullptr: off.
    const int32_t *pair_src;
    const int32_t *pair_col;
    long long pair_buf_off;
    // V2 min-sum bit gather (VNG, dv_max <= 4): the message pass records per
    // edge two bits (b2c <= 0, |b2c| == min1) in LDS, and one pass per bit
    // rebuilds its messages from its rows' aggregates and sums them in order.
    const uint2 *vn_rows;           // [n]: four u16 layout rows per bit, kpos order (0xFFFF: none); null: off
    // Hybrid shape (irregular codes): a bit's edges are padded to chunks of
    // four; vn_rows then holds the rows per chunk ([chunks], padding: row 0),
    // slot_meta2 each slot's padded edge position, and the gather walks bits
    // in degree order: vng_bits[i] = {bit, first chunk | dv << 24}.
    const uint2 *vng_bits;
    // Min-sum: the factor/offset can push |message| above its selected
    // minimum (|NMSA factor| > 1, negative offset, or NaN): clip every message.
    int ms_clip_later;
    // Hybrid min-sum whose row aggregates do not fit LDS beside the totals
    // (C5 R=0.5: m = 5120): rowAB lives in the workgroup's global scratch
    // (L2-resident) at this offset in doubles; -1: rows in LDS.
    long long rows_wg_offset;
    int rows_lds;                   // ... of which the leading rows_lds layout rows stay in LDS (m: all)
    int rows_lds_waves;             // = the rows of waves 0 .. rows_lds_waves - 1
    const int32_t *wave_rows;       // V2: first layout row of each wave (+ m)
    int rows_copy;                  // ... the others' message pass reads an LDS copy of its rows
    // Bank-aware bit labels (relabel.cpp; one-workgroup register shapes): the
    // graph's metadata and the frame codes use labels, llr / bits / posterior
    // the reference's bit ids.  nullptr: identity.
    const int32_t *col_orig;        // [n] label -> bit id (the frame codes the kernel reads are in labels)
    const int32_t *col_lab;         // [n] bit id -> label (outputs: bits / posterior in bit ids)
    // ... a frame the palette cannot hold is copied into label order at frame
    // setup, into its workgroup's scratch at this offset (doubles); -1: none
    long long llr_lab_wg_offset;
    // Per-frame decode span (nullable): [batch][2] s_memrealtime ticks (100 MHz)
    // at the frame's claim and at its results — the trial's own time inside the
    // batch (the reference times each trial's QKD_LDPC call, src/simulation.cpp:559-568)
    uint64_t *frame_clk;
    // SPA, one-workgroup register shapes (decoder_v2.hip, GATE): a parity-only
    // pass settles the exit test before the check-node scan of iteration it when
    // the scan of iteration it - 1 counted at most this many rows off their
    // syndrome bit, and at the iteration cap (< 0: never; the host's choice:
    // graph.hpp V2_EXIT_GATE).  Speed only: no result depends on it.
    int exit_gate;
};

// Frequency of s_memrealtime (gfx9: a constant 100 MHz clock).
constexpr double FRAME_CLK_HZ = 100.0e6;

// The persistent decoders' frame claim: the next frame of the launch's claim
// order (order.hip; results never depend on it).  >= batch: none left.
__device__ __forceinline__ int claim_frame(const DecodeArgs &a) {
    const int c = atomicAdd(a.frame_counter, 1);
    return (a.frame_order && c < a.batch) ? a.frame_order[c] : c;
}

// Dynamic LDS bytes / scratch doubles a variant needs for this shape.
size_t lds_bytes_for(int variant, int n, int m, int T);
long long scratch_doubles_for(int variant, int n, int m, int T, int EPL);

// Launch the persistent decoder: grid = `workgroups`, block = args.T.
hipError_t launch_decode(int variant, const DecodeArgs &a, int workgroups, size_t lds_bytes,
                         hipStream_t stream);
// Max resident workgroups per CU for (variant, alg, T, lds).
hipError_t occupancy(int variant, int alg, int T, size_t lds_bytes, int *blocks_per_cu);

// The environment variable `name` under the diagnostic switch QLDPC_DIAG=1, else NULL (plan.hip):
// the only way the library reads its QLDPC_* A/B knobs.
const char *qldpc_diag_env(const char *name);
constexpr size_t LDS_MAX_BYTES = 160 * 1024;
// Opt kernel k in to `bytes` of dynamic LDS (hipFuncAttributeMaxDynamicSharedMemorySize)
// on the current device.  The limit per (device, kernel) only ever rises,
// under one process-wide mutex: a
// per-launch value set by one thread could otherwise lower the limit between
// another thread's set and its launch (decoder.hip).
hipError_t allow_dynamic_lds(const void *k, size_t bytes);
// Dynamic LDS of the frame builders: the keys (+ punctured draws, the extended
// key) as bit words.  Beyond LDS_MAX_BYTES (plain frames: n > 655,360; rate-
// adapted: n > ~436k) the entries refuse the graph with QLDPC_EUNSUP.
inline size_t build_frames_lds(int n) { return 2 * (size_t)((n + 31) / 32) * sizeof(uint32_t); }
inline size_t build_frames_ra_lds(int n, int n_punct) {
    return (2 * (size_t)((n + 31) / 32) + (size_t)((n_punct + 31) / 32) + 2 * (size_t)((n + 63) / 64)) *
           sizeof(uint32_t);
}
// ... and of the per-party kernels (parties.hip): Alice's key (+ her punctured
// fill and the extended key, with a plan) for the syndrome; Bob's key alone.
inline size_t alice_syndrome_lds(int n, int n_punct /* < 0: no plan */) {
    const size_t nw = (size_t)((n + 31) / 32);
    if (n_punct < 0) return nw * sizeof(uint32_t);
    return (nw + (size_t)((n_punct + 31) / 32) + 2 * (size_t)((n + 63) / 64)) * sizeof(uint32_t);
}
inline size_t bob_frames_lds(int n) { return (size_t)((n + 31) / 32) * sizeof(uint32_t); }
// Threads per frame of the one-workgroup-per-frame byte kernels (frame build,
// claim weight, key compare): 256, or 1024 for frames of >= 32768 bits, whose
// batches (C4: 128 frames) leave most CUs idle at 4 waves per frame.
inline int aux_frame_threads(int n) { return n >= 32768 ? 1024 : 256; }
hipError_t launch_build_frames(int n, int m, int max_dc, const int32_t *ell_col, const int32_t *row_deg,
                               int batch, const uint8_t *alice, const uint8_t *bob, const double *log_p,
                               double *llr, uint8_t *synd, uint8_t *codes, double *palette, uint8_t *pal_ok,
                               const int32_t *col_orig, hipStream_t stream);

// One decode launch, decided once per call from the graph, the algorithm and
// the launch-time knobs (plan.hip launch_shape): which kernel runs, with how
// many threads and how much dynamic LDS.  Host only; every consumer (the
// occupancy query, the argument fill, the launch, qldpc_graph_plan) reads the
// choice from here and derives nothing of it again.
struct LaunchShape {
    int variant = 0, alg = 0;
    int threads = 0;       // per workgroup
    size_t lds_bytes = 0;  // dynamic LDS per workgroup
    // V2: the template arguments of decode_v2_kernel (decoder_v2.hip kernel_of)
    int R = 0, RG = 0, RL = 0;     // message slots per lane in VGPRs / global scratch / LDS
    int split_k = 1;               // workgroups per frame (1: not split)
    int part_lanes = REG_TSTRIDE;  // PL: a split part's lanes
    bool vng = false;              // min-sum bit gather (DecodeArgs::vn_rows)
    bool rglb = false;             // min-sum row aggregates (partly) in global scratch
    int rows_lds = 0;              // rows whose aggregates the LDS image holds
    int gcb = 0;                   // split exchange gather: bits per LDS chunk
    int lanes() const { return split_k * threads; }  // the lanes that run per frame
    // What the occupancy query asks (V2): the plain instantiation of the same
    // (R, RG, split, part lanes) at this launch's threads and LDS bytes, without
    // LDS message slots or the bit gather.  NOT the launched kernel whenever RL > 0
    // or vng: the workgroup counts of those launches come from this stand-in.
    LaunchShape occupancy_proxy() const {
        LaunchShape p = *this;
        p.RL = 0;
        p.vng = p.rglb = false;
        return p;
    }
    const char *variant_name() const;  // qldpc_graph_plan's: reg_lds .. v2, v2_hybrid, v2_split, fpl
    std::string name() const;          // e.g. v2<alg=0,R=40,RG=0,RL=5,split=1,pl=1024,vng=0,rglb=0>
};

// The V2 shape of a scalar description: RL and lds_bytes by the V2Layout fit tests
// (decoder_v2.hip; also the planners' fit queries, which read .lds_bytes / .RL).
struct V2ShapeQuery {
    int alg = 0, n = 0;
    int rows = 0;          // m, or the rows of a split frame's largest part
    int threads = 0;       // the workgroup's (split: one part's) lanes
    int split_k = 1;
    int R = 0, RG = 0;     // (split frames: every plan's slots share one LDS image)
    int rows_lds = -1;     // min-sum row aggregates kept in LDS on the hybrid shape (-1: all)
    int gcb = 0;
    bool want_vng = false, rglb = false;
};
LaunchShape v2_launch_shape(const V2ShapeQuery &q);
// Whether a V2 shape can run the min-sum bit gather (DecodeArgs::vn_rows):
// the dv <= 4 register shape, or the hybrid shape when the padded edge
// positions' two code bits fit the LDS byte area.
bool v2_vng_ok(int alg, int R, int RG, int split_k, int dv_max, int m);
constexpr int V2_VNG_DUMMY_CHUNKS = 64;  // hybrid: one scratch code byte per lane for dummy slots
// hipErrorInvalidValue: the shape has no instantiation, or the arguments lack what it reads.
hipError_t launch_decode_v2(const LaunchShape &s, const DecodeArgs &a, int workgroups, hipStream_t stream);
// Max resident workgroups per CU of the shape's kernel (callers pass occupancy_proxy()).
hipError_t occupancy_v2(const LaunchShape &s, int *blocks_per_cu);
hipError_t launch_palettize(int n, int nc, int batch, const double *llr, uint8_t *codes, double *palette,
                            uint8_t *pal_ok, const int32_t *col_orig, hipStream_t stream);
// Trial generator workspace (uint32 words) of `batch` trials.
size_t trials_scratch_words(int n, uint64_t n_err, int n_punct, int batch);
// The Xoshiro256 state after `draws` draws from a Xoshiro-cpp-seeded generator,
// by the jump matrix the trial generator's second wave uses (host; a check).
int xoshiro_jump_check(uint64_t seed, uint64_t draws, uint64_t *state_out);
hipError_t launch_trials(int n, uint64_t n_err, int batch, const uint64_t *seeds, uint64_t seed_add, uint8_t *alice,
                         uint8_t *bob, uint32_t *scratch, int n_punct, uint8_t *punct_alice, uint8_t *punct_bob,
                         hipStream_t stream);
hipError_t launch_build_frames_ra(int n, int m, const int32_t *ell_col, const int32_t *row_deg, const uint8_t *cls,
                                  const int32_t *src, int n_punct, int batch, const uint8_t *alice, const uint8_t *bob,
                                  const uint8_t *palice, const uint8_t *pbob, const double *log_p, uint8_t *alice_ext,
                                  double *llr, uint8_t *synd, uint8_t *codes, double *palette, uint8_t *pal_ok,
                                  const int32_t *col_orig, hipStream_t stream);
// ---- the per-party cut of the frame builders (parties.hip) --------------------
// Alice: the syndrome of her (extended) key.  cls == NULL: no plan, the key is
// the frame; else key_ext (nullable) receives the extended key as bytes.
hipError_t launch_alice_syndrome(int n, int m, const int32_t *ell_col, const int32_t *row_deg, const uint8_t *cls,
                                 const int32_t *src, int n_punct, int batch, const uint8_t *key,
                                 const uint8_t *fill, uint8_t *key_ext, uint8_t *synd, hipStream_t stream);
// Bob: the f64 LLRs (llr, nullable) and / or the V2 palette form (codes,
// nullable; with palette and pal_ok) of his key, as the fused builders write them.
hipError_t launch_bob_frames(int n, const uint8_t *cls, const int32_t *src, int batch, const uint8_t *key,
                             const double *log_p, double *llr, uint8_t *codes, double *palette, uint8_t *pal_ok,
                             const int32_t *col_orig, hipStream_t stream);
// The inverse of the extension: out[f][src[i]] = bits[f][i] where cls[i] == 0.
hipError_t launch_extract_key(int n, int n_key, const uint8_t *cls, const int32_t *src, int batch,
                              const uint8_t *bits, uint8_t *out, hipStream_t stream);
// ---- blind reconciliation's disclosure rounds (blind.hip) ------------------------
// list[0 .. *count) = the frames with synd_ok == 0, ascending (entries past the
// count are not written).
hipError_t launch_failed_frames(int batch, const uint8_t *synd_ok, int32_t *list, int32_t *count,
                                hipStream_t stream);
// Alice: out[j][i] = fill[list[j]][disc[i]] (list == NULL: frame j).
hipError_t launch_disclose(int n_punct, int n_list, const int32_t *list, const uint8_t *fill, int n_disc,
                           const int32_t *disc, uint8_t *out, hipStream_t stream);
// Bob: compact rows j < n_list of the round's LLRs and syndromes for the frames
// list[j] (NULL: frame j) of the [batch] inputs: launch_bob_frames' LLRs with the
// punctured positions of indices disc[i] pinned at vals[j][i] ? -DBL_MAX : DBL_MAX.
// Dynamic LDS: Bob's key as bit words and one byte per punctured index.
inline size_t round_frames_lds(int n, int n_punct) {
    return ((size_t)((n + 31) / 32) + (size_t)((n_punct + 3) / 4)) * sizeof(uint32_t);
}
hipError_t launch_round_frames(int n, int m, int batch, int n_punct, const uint8_t *cls, const int32_t *src,
                               int n_list, const int32_t *list, const uint8_t *key, const double *log_p,
                               const uint8_t *synd, int n_disc, const int32_t *disc, const uint8_t *vals,
                               double *llr, uint8_t *synd_ws, hipStream_t stream);
// ---- error estimation at the reconciliation stage (estimate.hip) ----------------
// weight[f] = the informative rows j (row_d[j] > 0: the row's effective degree,
// 0 = not informative) at which synd[f][j] differs from H * Bob's extended key
// (key bits at the plan's key positions, 0 elsewhere; cls / src nullable: no
// plan).  Dynamic LDS: the key, and with a plan the extended key, as bit words.
constexpr int EST_MAX_CLASSES = 64;  // degree classes the solve kernel takes as a kernel argument
inline size_t syndrome_weight_lds(int n, bool with_plan) {
    return ((size_t)((n + 31) / 32) + (with_plan ? 2 * (size_t)((n + 63) / 64) : 0)) * sizeof(uint32_t);
}
hipError_t launch_syndrome_weight(int n, int m, const int32_t *ell_col, const int32_t *row_deg, const int32_t *row_d,
                                  const uint8_t *cls, const int32_t *src, int batch, const uint8_t *key,
                                  const uint8_t *synd, int32_t *weight, hipStream_t stream);
// qber[f], log_p[f] (each nullable) from weight[f] and the class table (host
// arrays of n_classes <= EST_MAX_CLASSES entries): estimate_math.h, one thread per frame.
hipError_t launch_estimate_solve(int batch, int n_classes, const int32_t *degree, const int32_t *rows,
                                 const int32_t *weight, double q_min, double q_max, double *qber, double *log_p,
                                 hipStream_t stream);
// errors[f] = the key positions at which key[f] differs from bits[f]: with a
// plan #{i : cls[i] == 0, key[f][src[i]] != bits[f][i]}, without one the
// Hamming distance of the two n-byte rows.
hipError_t launch_corrected_errors(int n, const uint8_t *cls, const int32_t *src, int batch, const uint8_t *key,
                                   const uint8_t *bits, int32_t *errors, hipStream_t stream);
// ---- symmetric blind rounds: per-frame positions (select.hip, blind.hip) --------
// pos[f][first .. first + count) = the `count` candidate positions of frame
// f = list[j] (NULL: f = j) with the smallest (|posterior| as 63 bits, index), in
// that order; candidates are the positions that are neither shortened
// (cls[i] == 2; cls nullable) nor in pos[f][0 .. first).  pos is [batch][cap].
constexpr int SELECT_MAX = 4096;  // winners sorted in LDS (QLDPC_SELECT_MAX)
size_t select_lds(int n, int count);
hipError_t launch_select(int n, int batch, const uint8_t *cls, int n_list, const int32_t *list, const double *post,
                         int first, int count, int32_t *pos, int cap, hipStream_t stream);
// Alice: out[j][i] = ext[f][pos[f][first + i]] & 1 for i < count (ext rows of ext_stride bytes).
hipError_t launch_disclose_positions(int n, int n_list, const int32_t *list, const uint8_t *ext, size_t ext_stride,
                                     const int32_t *pos, int cap, int first, int count, uint8_t *out,
                                     hipStream_t stream);
// Bob: launch_round_frames with the positions pos[f][0 .. n_disc) pinned at
// vals[j][i] ? -DBL_MAX : DBL_MAX, whatever their class (cls / src nullable: no plan).
// Dynamic LDS: the key, the pinned positions and their bits as bit words.
inline size_t positions_frames_lds(int n) { return 3 * (size_t)((n + 31) / 32) * sizeof(uint32_t); }
hipError_t launch_positions_frames(int n, int m, int batch, const uint8_t *cls, const int32_t *src, int n_list,
                                   const int32_t *list, const uint8_t *key, const double *log_p, const uint8_t *synd,
                                   int n_disc, const int32_t *pos, int cap, const uint8_t *vals, double *llr,
                                   uint8_t *synd_ws, hipStream_t stream);
// Rows list[j] of the [batch] outputs <- compact row j (cpost / post nullable together).
hipError_t launch_round_scatter(int n, int batch, int n_list, const int32_t *list, const uint8_t *cbits,
                                const uint32_t *citers, const uint8_t *cok, const double *cpost, uint8_t *bits,
                                uint32_t *iters, uint8_t *ok, double *post, hipStream_t stream);
// ---- key verification and privacy amplification (privacy.hip) ----------------------
// out[f][i] = XOR_j seed[i + key_len - 1 - j] & keys[f][j] for i < out_lens[f]
// (NULL: out_len; clamped into [0, out_len]), 0 for the rest of the row.  A
// workgroup hashes HASH_TILE outputs of HASH_FRAMES frames.  Dynamic LDS: the
// frames' keys as bit words (rows padded to 4 words) and the tile's seed window.
constexpr int HASH_THREADS = 256, HASH_TILE = 1024, HASH_FRAMES = 4;
constexpr int hash_seed_words(int key_len) { return 4 * ((key_len + 127) / 128) + HASH_TILE / 32; }
inline size_t toeplitz_hash_lds(int key_len) {
    const size_t kw4 = 4 * (((size_t)key_len + 127) / 128);  // (as hash_seed_words, whatever the key's length)
    return ((size_t)HASH_FRAMES * kw4 + kw4 + HASH_TILE / 32) * sizeof(uint32_t);
}
// The grid is (frame groups, output tiles): HIP bounds x * threads below 2^32 and y by 65535.
inline bool toeplitz_hash_grid_ok(int batch, int out_len) {
    return ((long long)batch + HASH_FRAMES - 1) / HASH_FRAMES * HASH_THREADS < (1ll << 32) &&
           ((long long)out_len + HASH_TILE - 1) / HASH_TILE <= 65535;
}
hipError_t launch_toeplitz_hash(int batch, int key_len, long long key_stride, const uint8_t *keys, int out_len,
                                const uint8_t *seed, const int32_t *out_lens, uint8_t *out, hipStream_t stream);
// ---- the hash of one long block (privacy_block.hip) --------------------------------
// out[i] = XOR_j seed[i + L - 1 - j] & x[j] for the block x = rows list[0 .. n_list)
// (NULL: rows 0 ..) of keys, concatenated, L = n_list * key_len: an exact cyclic
// convolution of N = 2^k >= L + out_len - 1 points by a number-theoretic transform.
// The lowest NTT_TILE_LOG stages run on a workgroup's LDS tile, the stages above
// in strided passes of at most NTT_PASS_STAGES stages.  The workspace holds the
// two arrays and the twiddle table, N words each, from a 16-byte boundary.
constexpr int NTT_TILE_LOG = 12, NTT_PASS_STAGES = 7, NTT_MAX_LOG = 27;
// k, or -1 where L + r - 1 is beyond 2^NTT_MAX_LOG (L, r >= 1)
inline int toeplitz_block_log2(long long L, long long r) {
    if (L < 1 || r < 1 || L > (1ll << NTT_MAX_LOG) || r > (1ll << NTT_MAX_LOG) || L + r - 1 > (1ll << NTT_MAX_LOG))
        return -1;
    int k = 0;
    while ((1ll << k) < L + r - 1) ++k;
    return k;
}
inline size_t toeplitz_block_ws(int k) { return 3 * sizeof(uint32_t) * ((size_t)1 << k) + 16; }
hipError_t launch_toeplitz_block(int n_list, const int32_t *list, int key_len, long long key_stride,
                                 const uint8_t *keys, long long out_len, const uint8_t *seed, uint8_t *out, void *ws,
                                 hipStream_t stream);
// Claim order of a batch: frames by ascending weight of the channel decision's
// syndrome mismatch (order.hip).  llr is read only for frames without codes.
size_t frame_weight_lds(int n);
hipError_t launch_frame_order(int n, int m, const int32_t *ell_col, const int32_t *row_deg, int batch,
                              const uint8_t *synd, const double *llr, const uint8_t *codes,
                              const double *palette, const uint8_t *pal_ok, int32_t *weight, int32_t *order,
                              const int32_t *col_orig, hipStream_t stream);
// ---- frame-per-lane decoder (decoder_fpl.hip) ---------------------------------
// A chunk of `tiles` tiles of 64 frames, lane = frame.  Per tile: messages
// C[E][64] at bit_nodes (CSC) positions, totals T[n][64], channel LLRs
// L[n][64], and one 64-bit lane mask per bit (hard decision) and per row
// (target syndrome).  Tile t, slot s holds the frame at position
// frame0 + 64 t + s of the deal (frame_order, or index order).
constexpr int FPL_LANES = 64;
constexpr int FPL_CN_WAVES = 4;   // rows per workgroup of the check-node pass
constexpr int FPL_BIT_RUN = 4;    // consecutive bits per wave of the bit pass
// Rows of at most this many edges keep their per-edge values (SPA: tanh(b/2),
// min-sum: b) in registers between the two sweeps of the check-node pass;
// longer rows stash them in C (SPA) or recompute them (min-sum).
constexpr int FPL_ROW_CAP = 32;
// The check-node pass is one launch per class of row lengths (0, <= 4, 8, 12,
// 16, 24, 32 edges, longer), each instantiation with the registers its own
// bucket needs: rows[] lists the rows by class, class c at
// [class_off[c], class_off[c + 1]).
constexpr int FPL_CLASSES = 8;
constexpr int FPL_CLASS_CAP[FPL_CLASSES] = {0, 4, 8, 12, 16, 24, 32, 1 << 30};
inline int fpl_row_class(int deg) {
    int c = 0;
    while (deg > FPL_CLASS_CAP[c]) ++c;
    return c;
}
struct FplArgs {
    int n, m, E;
    const int32_t *rows;     // [m] rows by class
    int class_off[FPL_CLASSES + 1];
    const int32_t *row_ptr;  // [m + 1] check_nodes
    const int32_t *col_idx;  // [E]
    const int32_t *cslot;    // [E] position of the row-major edge in bit_nodes order
    const int32_t *col_ptr;  // [n + 1] bit_nodes
    int alg, max_it, thr_on;
    double thr, primary, secondary;
    int tiles, frames, frame0;   // this chunk: tiles, frames (<= 64 tiles), first deal position
    const int32_t *frame_order;  // [batch] deal position -> frame; nullptr: index order
    const double *llr;
    const uint8_t *synd;
    uint8_t *bits;
    uint32_t *iters;
    uint8_t *ok;
    double *post;         // nullable
    uint64_t *frame_clk;  // nullable
    double *C, *T, *L;    // [tiles][E | n | n][64]
    uint64_t *hard;       // [tiles][n]
    uint64_t *syn;        // [tiles][m]
    uint64_t *active;     // [tiles] lanes still decoding
    uint64_t *flags;      // [tiles] lanes with a mismatched row in the pass just run
};
// Workspace bytes of one tile (8-byte units: doubles then masks).
inline size_t fpl_tile_words(int n, int m, int E) {
    return ((size_t)E + 2 * (size_t)n) * FPL_LANES + (size_t)n + (size_t)(m > 0 ? m : 1) + 2;
}
// Workgroups of the check-node pass for one tile: FPL_CN_WAVES rows each, per class.
inline int fpl_cn_grid(const int *class_off) {
    int g = 0;
    for (int c = 0; c < FPL_CLASSES; ++c) g += (class_off[c + 1] - class_off[c] + FPL_CN_WAVES - 1) / FPL_CN_WAVES;
    return g;
}
// The per-iteration trace of a frame-per-lane decode (qldpc_decode_trace_batch*):
// row `it` of a frame is written after the bit pass of iteration `it` while
// the frame's lane is still in its tile's active mask, and by nothing else.
constexpr int FPL_TRACE_ROWS = 8;  // rows per wave of the unsatisfied-row count
struct FplTrace {
    uint32_t *unsat = nullptr;  // [batch][max_it] rows off their syndrome bit; nullable
    double *post = nullptr;     // [batch][max_it][n] totals; nullable
    uint32_t *cnt = nullptr;    // [tiles][64] per-lane counters of the count in flight (zero between launches)
    bool on() const { return unsat || post; }
};
// Enqueue one chunk's whole decode: load transposes, max_it iterations of
// (check-node pass, settle, bit pass), the closing parity / settle, store
// transposes.  With a trace, each bit pass is followed by the count of
// unsatisfied rows (two launches) and / or the store of the totals' row.
// Nothing in it waits on another workgroup.
hipError_t launch_fpl_chunk(const FplArgs &a, const FplTrace &trace, hipStream_t stream);

// The host-computed constants of the SPA clipped forms (capi.hip spa_clip()):
// what a decode launch hands its kernel and what the math self-test evaluates
// fn 8 / fn 9 with.
struct SpaClip {
    double thr;    // the clip threshold, +inf when clipping is off
    double lim;    // min(thr, 44): tanh(+-b/2) = +-t_lim for |b| >= lim, clipped or not
    double t_lim;  // glibc tanh(lim / 2.)  (1 for lim = 44)
    double c_top;  // glibc 2. * atanh(1 - 2^-53)
};

hipError_t launch_math_selftest(int fn, const SpaClip &clip, int count, const double *in, double *out,
                                hipStream_t stream);
hipError_t launch_keys_match(int batch, int n, const uint8_t *alice, const uint8_t *bits,
                             uint8_t *match, hipStream_t stream);

}  // namespace qldpc
