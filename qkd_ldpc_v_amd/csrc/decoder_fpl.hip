// decoder_fpl.hip — the frame-per-lane decoder: lanes are frames.
//
// A batch is cut into tiles of 64 frames.  One wave works on one row (or a
// run of bits) of one tile: the graph walk — row bounds, bit ids, bit_nodes
// positions — is wave-uniform and comes by scalar loads, and every message,
// total and LLR access is 64 consecutive doubles, one per frame.  An
// iteration is a few ordinary launches on the caller's stream:
//
//   check-node pass   one wave per (tile, row), one launch per class of row
//                     lengths: parity of the row's decisions
//                     (scalar XOR of 64-bit lane masks), then the row's
//                     messages from b = T[bit] - C[f] (clipped), written to C
//   settle            one wave per tile: the lanes none of whose rows
//                     mismatched leave the tile's active mask with their
//                     iteration count
//   bit pass          one wave per (tile, run of bits): T = L + sum C in
//                     bit_nodes order, decisions by ballot
//   trace (on demand) after the bit pass, for the lanes still active: the
//                     count of rows off their syndrome bit (a count launch
//                     and a one-wave-per-tile flush) and / or the totals' row
//
// No kernel here waits on memory another workgroup writes: ordering comes
// from stream order alone, so the decode cannot stall on residency, CU masks
// or co-tenants.  A tile with no active lane returns at once.
//
// Semantics restate oracle/ldpc_oracle.c decode_impl (which cites the
// reference): iteration 0 reads the unclipped LLRs; C is clipped when
// written, b when recomputed, both only with the threshold on; a decision is
// 1 iff total <= 0; SPA / SPA-LIN / NMSA / OMSA exit on the parity of the bit
// pass's decisions, taken at the head of the next check-node pass (a closing
// parity launch follows the last iteration); ANMSA / AOMSA start from the
// channel decision, test each row inside the check-node pass (mismatched
// rows take the secondary factor) and exit right after a pass without a
// mismatch, before the bit pass.  A settled lane is masked in every kernel
// that writes T, the decision masks, iters or ok.
#include "decoder_common.hpp"

namespace qldpc {

namespace {

using dev::agg_init;
using dev::agg_push;
using dev::atanh_lin;
using dev::clip_msg;
using dev::MinAgg;
using dev::tanh_lin;

// The frame in slot s of tile t of this chunk, or -1 past the batch's end.
__device__ __forceinline__ long long fpl_frame(const FplArgs &a, int tile, int slot) {
    const int pos = tile * FPL_LANES + slot;
    if (pos >= a.frames) return -1;
    return a.frame_order ? a.frame_order[a.frame0 + pos] : a.frame0 + pos;
}

// ---- in: [frame][bit] LLRs -> L[tile][bit][64], T = 0, channel decisions -----
// 64 frames x 64 bits through LDS: rows are read along bits (512 contiguous
// bytes of one frame) and written along frames.
__global__ void __launch_bounds__(256) fpl_load_llr(FplArgs a) {
    __shared__ double sh[FPL_LANES][FPL_LANES + 1];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int tile = blockIdx.y, b0 = blockIdx.x * FPL_LANES;
    for (int r = 0; r < FPL_LANES / 4; ++r) {
        const int slot = r * 4 + wave;
        const long long fr = fpl_frame(a, tile, slot);
        const int bit = b0 + lane;
        sh[slot][lane] = (fr >= 0 && bit < a.n) ? a.llr[(size_t)fr * a.n + bit] : 0.0;
    }
    __syncthreads();
    const bool valid = fpl_frame(a, tile, lane) >= 0;
    for (int r = 0; r < FPL_LANES / 4; ++r) {
        const int bl = r * 4 + wave, bit = b0 + bl;
        if (bit >= a.n) continue;  // (wave-uniform)
        const double v = sh[lane][bl];
        const size_t at = ((size_t)tile * a.n + bit) * FPL_LANES + lane;
        a.L[at] = v;
        a.T[at] = 0.0;
        const uint64_t z = __ballot(valid && v <= 0);
        if (lane == 0) a.hard[(size_t)tile * a.n + bit] = z;
    }
}

// ---- in: [frame][row] syndrome bytes -> one lane mask per row; tile state -----
__global__ void __launch_bounds__(256) fpl_load_synd(FplArgs a) {
    const int tile = blockIdx.y;
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const int left = a.frames - tile * FPL_LANES;
        a.active[tile] = left >= FPL_LANES ? ~0ull : (left > 0 ? (1ull << left) - 1 : 0ull);
        a.flags[tile] = 0;
    }
    if (j >= a.m) return;
    uint64_t mask = 0;
    for (int s = 0; s < FPL_LANES; ++s) {
        const long long fr = fpl_frame(a, tile, s);  // (uniform)
        if (fr < 0) break;
        mask |= (uint64_t)(a.synd[(size_t)fr * a.m + j] & 1) << s;  // 256 contiguous bytes per frame
    }
    a.syn[(size_t)tile * a.m + j] = mask;
}

// The row a wave works on: the lanes (frames) whose decisions' parity over the
// row differs from their syndrome bit.  Lane k fetches the decision mask of the
// row's k-th bit (one round trip for rows of up to 64 edges instead of one per
// edge), then a butterfly XOR leaves the parity in every lane.
__device__ __forceinline__ uint64_t row_mismatch(const FplArgs &a, int tile, int j, int e0, int e1, int lane) {
    const uint64_t *hard = a.hard + (size_t)tile * a.n;
    uint64_t par = 0;
    for (int e = e0 + lane; e < e1; e += FPL_LANES) par ^= hard[a.col_idx[e]];
    uint32_t lo = (uint32_t)par, hi = (uint32_t)(par >> 32);
    for (int o = 32; o > 0; o >>= 1) {
        lo ^= (uint32_t)__shfl_xor((int)lo, o, FPL_LANES);
        hi ^= (uint32_t)__shfl_xor((int)hi, o, FPL_LANES);
    }
    return (((uint64_t)hi << 32) | lo) ^ a.syn[(size_t)tile * a.m + j];
}

// ---- check-node pass ----------------------------------------------------------
// ALG: 0 SPA, 1 SPA-LIN, 2 NMSA, 3 OMSA, 4 ANMSA, 5 AOMSA.
template <int ALG>
struct CnMath {
    static constexpr bool SPA_FAMILY = ALG <= 1, NORMALIZED = ALG == 2 || ALG == 4, ADAPTIVE = ALG >= 4;
    static __device__ __forceinline__ double th(double b) {
        return ALG == 0 ? ql_exact::tanh_half_dec(b) : tanh_lin(b / 2.);
    }
    static __device__ __forceinline__ double ath(double p) {
        return ALG == 0 ? ql_exact::atanh2_dec(p) : 2. * atanh_lin(p);
    }
    // a min-sum message from the row's aggregate and the edge's own input
    static __device__ __forceinline__ double msg(double b, const MinAgg &g, double sign_prod, double factor) {
        const double prod = sign_prod * ((b > 0) ? 1. : -1.);
        const double sel = (fabs(b) == g.m1) ? g.m2 : g.m1;
        if (NORMALIZED) return factor * prod * sel;
        const double diff = sel - factor;
        return prod * ((diff < 0.) ? 0. : diff);
    }
};

// A row of at most B <= FPL_ROW_CAP edges: its inputs are fetched by B
// unconditional loads (positions past the row's end repeat its last edge), so
// all of them are in flight together, and its per-edge values (SPA: tanh(b/2),
// min-sum: b) stay in registers between the two sweeps.
template <int ALG, int B>
__device__ __forceinline__ void cn_row_reg(const FplArgs &a, int it, int tile, int lane, int e0, int deg,
                                           bool synd_bit, bool mismatch) {
    using M = CnMath<ALG>;
    double *const C = a.C + (size_t)tile * a.E * FPL_LANES + lane;
    const bool clip = a.thr_on != 0;
    const double thr = a.thr;
    int f[B];
    double v[B];
    if (it == 0) {  // the channel LLRs, unclipped
        const double *const L = a.L + (size_t)tile * a.n * FPL_LANES + lane;
#pragma unroll
        for (int k = 0; k < B; ++k) {
            const int e = e0 + (k < deg ? k : deg - 1);
            f[k] = a.cslot[e];
            v[k] = L[(size_t)a.col_idx[e] * FPL_LANES];
        }
    } else {  // total - c2b, clipped
        const double *const T = a.T + (size_t)tile * a.n * FPL_LANES + lane;
        double c[B];
#pragma unroll
        for (int k = 0; k < B; ++k) {
            const int e = e0 + (k < deg ? k : deg - 1);
            f[k] = a.cslot[e];
            v[k] = T[(size_t)a.col_idx[e] * FPL_LANES];
            c[k] = C[(size_t)f[k] * FPL_LANES];
        }
#pragma unroll
        for (int k = 0; k < B; ++k) {
            const double b = v[k] - c[k];
            v[k] = clip ? clip_msg(b, thr) : b;
        }
    }
    auto put = [&](int k, double c) { C[(size_t)f[k] * FPL_LANES] = clip ? clip_msg(c, thr) : c; };
    if constexpr (M::SPA_FAMILY) {
        double row_prod = synd_bit ? -1. : 1.;
#pragma unroll
        for (int k = 0; k < B; ++k)
            if (k < deg) {
                v[k] = M::th(v[k]);
                row_prod *= v[k];
            }
#pragma unroll
        for (int k = 0; k < B; ++k)
            if (k < deg) put(k, M::ath(row_prod / v[k]));
    } else {
        MinAgg g;
        agg_init(g);
#pragma unroll
        for (int k = 0; k < B; ++k)
            if (k < deg) agg_push(g, v[k]);
        const double sign_prod = (synd_bit ? -1. : 1.) * (g.neg ? -1. : 1.);
        const double factor = (M::ADAPTIVE && mismatch) ? a.secondary : a.primary;
#pragma unroll
        for (int k = 0; k < B; ++k)
            if (k < deg) put(k, M::msg(v[k], g, sign_prod, factor));
    }
}

// A row past FPL_ROW_CAP: SPA's tanh(b / 2) waits in the edge's own C slot
// between the sweeps; min-sum forms b again (its C slot is overwritten only
// in the second sweep).
template <int ALG>
__device__ __forceinline__ void cn_row_long(const FplArgs &a, int it, int tile, int lane, int e0, int e1,
                                            bool synd_bit, bool mismatch) {
    using M = CnMath<ALG>;
    double *const C = a.C + (size_t)tile * a.E * FPL_LANES + lane;
    const double *const T = (it == 0 ? a.L : a.T) + (size_t)tile * a.n * FPL_LANES + lane;
    const bool clip = a.thr_on != 0;
    const double thr = a.thr;
    auto b2c = [&](int e) -> double {
        const double t = T[(size_t)a.col_idx[e] * FPL_LANES];
        if (it == 0) return t;
        const double b = t - C[(size_t)a.cslot[e] * FPL_LANES];
        return clip ? clip_msg(b, thr) : b;
    };
    auto put = [&](int e, double c) { C[(size_t)a.cslot[e] * FPL_LANES] = clip ? clip_msg(c, thr) : c; };
    if constexpr (M::SPA_FAMILY) {
        double row_prod = synd_bit ? -1. : 1.;
        for (int e = e0; e < e1; ++e) {
            const double t = M::th(b2c(e));
            C[(size_t)a.cslot[e] * FPL_LANES] = t;
            row_prod *= t;
        }
        for (int e = e0; e < e1; ++e) put(e, M::ath(row_prod / C[(size_t)a.cslot[e] * FPL_LANES]));
    } else {
        MinAgg g;
        agg_init(g);
        for (int e = e0; e < e1; ++e) agg_push(g, b2c(e));
        const double sign_prod = (synd_bit ? -1. : 1.) * (g.neg ? -1. : 1.);
        const double factor = (M::ADAPTIVE && mismatch) ? a.secondary : a.primary;
        for (int e = e0; e < e1; ++e) put(e, M::msg(b2c(e), g, sign_prod, factor));
    }
}

// One launch per class of row lengths (FPL_CLASS_CAP), so that each
// instantiation's registers — and with them the waves a SIMD holds — are those
// of its own bucket.  B: the class's cap (0: empty rows, parity only;
// > FPL_ROW_CAP: the long rows).
template <int ALG, int B>
__global__ void __launch_bounds__(64 * FPL_CN_WAVES) fpl_cn(FplArgs a, int it, int r0, int r1, int stamp) {
    constexpr bool ADAPTIVE = ALG >= 4;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const int tile = blockIdx.y;
    const int r = r0 + blockIdx.x * FPL_CN_WAVES + wave;
    if (r >= r1) return;
    const uint64_t act = a.active[tile];
    if (!act) return;
    const int j = a.rows[r];
    const int e0 = a.row_ptr[j], e1 = a.row_ptr[j + 1];
    // (stamp: the first launch of iteration 0; its first wave stamps the tile's frames)
    if (stamp && r == r0 && a.frame_clk && ((act >> lane) & 1)) {
        const long long fr = fpl_frame(a, tile, lane);
        if (fr >= 0) a.frame_clk[2 * (size_t)fr] = __builtin_amdgcn_s_memrealtime();
    }
    uint64_t mis = 0;
    if (ADAPTIVE || it > 0) {
        mis = row_mismatch(a, tile, j, e0, e1, lane) & act;
        if (mis && lane == 0) atomicOr((unsigned long long *)&a.flags[tile], (unsigned long long)mis);
    }
    if constexpr (B > 0) {
        if (e0 == e1 || !((act >> lane) & 1)) return;
        const bool synd_bit = (a.syn[(size_t)tile * a.m + j] >> lane) & 1;
        const bool mismatch = (mis >> lane) & 1;
        if constexpr (B <= FPL_ROW_CAP) cn_row_reg<ALG, B>(a, it, tile, lane, e0, e1 - e0, synd_bit, mismatch);
        else cn_row_long<ALG>(a, it, tile, lane, e0, e1, synd_bit, mismatch);
    }
}

// The closing parity of SPA / SPA-LIN / NMSA / OMSA: the check-node pass's head alone.
__global__ void __launch_bounds__(64 * FPL_CN_WAVES) fpl_parity(FplArgs a) {
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int tile = blockIdx.y;
    const int j = blockIdx.x * FPL_CN_WAVES + wave;
    if (j >= a.m) return;
    const uint64_t act = a.active[tile];
    if (!act) return;
    const uint64_t mis = row_mismatch(a, tile, j, a.row_ptr[j], a.row_ptr[j + 1], threadIdx.x & 63) & act;
    if (mis && (threadIdx.x & 63) == 0) atomicOr((unsigned long long *)&a.flags[tile], (unsigned long long)mis);
}

// ---- settle: one wave per tile --------------------------------------------------
// Active lanes without a flagged row leave with exit_iters iterations and
// syndromes_match = 1 (use_flags); `last` ends the others at max_it without a
// match.  The flags are cleared for the next pass.
__global__ void __launch_bounds__(64) fpl_settle(FplArgs a, int exit_iters, int use_flags, int last) {
    const int tile = blockIdx.x, lane = threadIdx.x;
    const uint64_t act = a.active[tile];
    if (!act) return;
    const uint64_t fl = a.flags[tile];
    const uint64_t done = use_flags ? act & ~fl : 0ull;
    const uint64_t left = act & ~done;
    const bool mine_done = (done >> lane) & 1, mine_left = (left >> lane) & 1;
    if (mine_done || (last && mine_left)) {
        const long long fr = fpl_frame(a, tile, lane);
        if (fr >= 0) {
            a.iters[fr] = (uint32_t)(mine_done ? exit_iters : a.max_it);
            a.ok[fr] = mine_done ? 1 : 0;
            if (a.frame_clk) a.frame_clk[2 * (size_t)fr + 1] = __builtin_amdgcn_s_memrealtime();
        }
    }
    if (lane == 0) {
        a.active[tile] = last ? 0ull : left;
        a.flags[tile] = 0;
    }
}

// ---- bit pass: total = llr + messages in bit_nodes order, decisions -------------
__global__ void __launch_bounds__(256) fpl_bit(FplArgs a) {
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const int tile = blockIdx.y;
    const uint64_t act = a.active[tile];
    if (!act) return;
    const bool on = (act >> lane) & 1;
    const int i0 = (blockIdx.x * 4 + wave) * FPL_BIT_RUN;
    if (i0 >= a.n) return;
    const double *const C = a.C + (size_t)tile * a.E * FPL_LANES + lane;
    // the run's bounds and LLRs first (positions past n repeat bit n - 1), so
    // their loads are in flight together
    int fb[FPL_BIT_RUN + 1];
    double l[FPL_BIT_RUN];
#pragma unroll
    for (int r = 0; r <= FPL_BIT_RUN; ++r) fb[r] = a.col_ptr[min(i0 + r, a.n)];
#pragma unroll
    for (int r = 0; r < FPL_BIT_RUN; ++r)
        l[r] = on ? a.L[((size_t)tile * a.n + min(i0 + r, a.n - 1)) * FPL_LANES + lane] : 0.0;
#pragma unroll
    for (int r = 0; r < FPL_BIT_RUN; ++r) {
        const int i = i0 + r;
        if (i >= a.n) break;
        double acc = l[r];
        if (on) {
            // four messages per round trip, added in bit_nodes order
            for (int f = fb[r]; f < fb[r + 1]; f += 4) {
                const int last = fb[r + 1] - 1;
                const double c0 = C[(size_t)f * FPL_LANES], c1 = C[(size_t)min(f + 1, last) * FPL_LANES];
                const double c2 = C[(size_t)min(f + 2, last) * FPL_LANES], c3 = C[(size_t)min(f + 3, last) * FPL_LANES];
                acc = acc + c0;
                if (f + 1 <= last) acc = acc + c1;
                if (f + 2 <= last) acc = acc + c2;
                if (f + 3 <= last) acc = acc + c3;
            }
            a.T[((size_t)tile * a.n + i) * FPL_LANES + lane] = acc;
        }
        const uint64_t z = __ballot(on && acc <= 0);
        if (lane == 0) {
            uint64_t *h = a.hard + (size_t)tile * a.n + i;
            *h = (*h & ~act) | z;
        }
    }
}

// ---- out: decision masks -> [frame][bit] bytes; T -> [frame][bit] posteriors ----
__global__ void __launch_bounds__(256) fpl_store_bits(FplArgs a) {
    const int tile = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    const uint64_t mask = a.hard[(size_t)tile * a.n + i];
    for (int s = 0; s < FPL_LANES; ++s) {
        const long long fr = fpl_frame(a, tile, s);  // (uniform)
        if (fr < 0) break;
        a.bits[(size_t)fr * a.n + i] = (uint8_t)((mask >> s) & 1);  // 256 contiguous bytes per frame
    }
}

// 64 bits x 64 frames of T through LDS, read along frames and written along
// bits: frame fr's 64 totals go to dst[fr * stride + bit], for the slots in `lanes`.
__device__ __forceinline__ void fpl_post_rows(const FplArgs &a, double *dst, size_t stride, uint64_t lanes) {
    __shared__ double sh[FPL_LANES][FPL_LANES + 1];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int tile = blockIdx.y, b0 = blockIdx.x * FPL_LANES;
    for (int r = 0; r < FPL_LANES / 4; ++r) {
        const int bl = r * 4 + wave, bit = b0 + bl;
        sh[lane][bl] = bit < a.n ? a.T[((size_t)tile * a.n + bit) * FPL_LANES + lane] : 0.0;
    }
    __syncthreads();
    for (int r = 0; r < FPL_LANES / 4; ++r) {
        const int slot = r * 4 + wave;
        const long long fr = fpl_frame(a, tile, slot);
        const int bit = b0 + lane;
        if (fr >= 0 && ((lanes >> slot) & 1) && bit < a.n) dst[(size_t)fr * stride + bit] = sh[slot][lane];
    }
}

__global__ void __launch_bounds__(256) fpl_store_post(FplArgs a) { fpl_post_rows(a, a.post, (size_t)a.n, ~0ull); }

// ---- trace: what the bit pass of iteration `it` left, for the lanes still active ----
// The count of rows off their syndrome bit.  A wave walks FPL_TRACE_ROWS rows of
// the tile (empty rows too: their parity is 0) and each lane sums its own bit of
// the mismatch masks; the workgroup's waves combine in LDS and one atomic add per
// lane with a non-zero sum goes to the tile's counters, which fpl_trace_flush
// reads in the next launch.
__global__ void __launch_bounds__(256) fpl_trace_count(FplArgs a, FplTrace t) {
    __shared__ uint32_t sh[4][FPL_LANES];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const int tile = blockIdx.y;
    const uint64_t act = a.active[tile];
    if (!act) return;  // (the whole workgroup: one tile)
    const int j0 = (blockIdx.x * 4 + wave) * FPL_TRACE_ROWS;
    uint32_t sum = 0;
    for (int j = j0; j < min(j0 + FPL_TRACE_ROWS, a.m); ++j) {
        const uint64_t mis = row_mismatch(a, tile, j, a.row_ptr[j], a.row_ptr[j + 1], lane) & act;
        sum += (uint32_t)((mis >> lane) & 1);
    }
    sh[wave][lane] = sum;
    __syncthreads();
    if (wave == 0) {
        sum = sh[0][lane] + sh[1][lane] + sh[2][lane] + sh[3][lane];
        if (sum) atomicAdd(&t.cnt[(size_t)tile * FPL_LANES + lane], sum);
    }
}

// One wave per tile: the counters to unsat[frame][it] for the active lanes, and back to zero.
__global__ void __launch_bounds__(64) fpl_trace_flush(FplArgs a, FplTrace t, int it) {
    const int tile = blockIdx.x, lane = threadIdx.x;
    const uint64_t act = a.active[tile];
    if (!act) return;
    uint32_t *const c = t.cnt + (size_t)tile * FPL_LANES + lane;
    if ((act >> lane) & 1) {
        const long long fr = fpl_frame(a, tile, lane);
        if (fr >= 0) t.unsat[(size_t)fr * a.max_it + it] = *c;
    }
    *c = 0;
}

// The totals to post[frame][it][bit]: fpl_store_post's transpose, active lanes only.
__global__ void __launch_bounds__(256) fpl_trace_post(FplArgs a, FplTrace t, int it) {
    const uint64_t act = a.active[blockIdx.y];
    if (!act) return;  // (the whole workgroup: one tile)
    fpl_post_rows(a, t.post + (size_t)it * a.n, (size_t)a.max_it * a.n, act);
}

template <int ALG, int B>
void launch_cn_class(const FplArgs &a, int it, int c, bool &first, hipStream_t s) {
    const int r0 = a.class_off[c], r1 = a.class_off[c + 1];
    if (r1 == r0) return;
    if (B == 0 && !(ALG >= 4 || it > 0)) return;  // empty rows: only their parity test
    const dim3 grid((r1 - r0 + FPL_CN_WAVES - 1) / FPL_CN_WAVES, (unsigned)a.tiles);
    hipLaunchKernelGGL((fpl_cn<ALG, B>), grid, dim3(64 * FPL_CN_WAVES), 0, s, a, it, r0, r1, (it == 0 && first) ? 1 : 0);
    first = false;
}
template <int ALG>
void launch_cn(const FplArgs &a, int it, hipStream_t s) {
    static_assert(FPL_CLASSES == 8 && FPL_CLASS_CAP[6] == FPL_ROW_CAP, "one instantiation per class");
    bool first = true;
    launch_cn_class<ALG, 0>(a, it, 0, first, s);
    launch_cn_class<ALG, 4>(a, it, 1, first, s);
    launch_cn_class<ALG, 8>(a, it, 2, first, s);
    launch_cn_class<ALG, 12>(a, it, 3, first, s);
    launch_cn_class<ALG, 16>(a, it, 4, first, s);
    launch_cn_class<ALG, 24>(a, it, 5, first, s);
    launch_cn_class<ALG, 32>(a, it, 6, first, s);
    launch_cn_class<ALG, 64>(a, it, 7, first, s);
}

}  // namespace

hipError_t launch_fpl_chunk(const FplArgs &a, const FplTrace &trace, hipStream_t s) {
    if (a.tiles <= 0 || a.frames <= 0) return hipSuccess;
    if (trace.unsat && !trace.cnt) return hipErrorInvalidValue;
    const dim3 g_cnt(((a.m > 0 ? a.m : 1) + 4 * FPL_TRACE_ROWS - 1) / (4 * FPL_TRACE_ROWS), (unsigned)a.tiles);
    const unsigned tiles = (unsigned)a.tiles;
    const bool adaptive = a.alg >= 4;
    const dim3 g_llr((a.n + FPL_LANES - 1) / FPL_LANES, tiles), g_n256((a.n + 255) / 256, tiles);
    const dim3 g_m256(a.m > 0 ? (a.m + 255) / 256 : 1, tiles);
    const dim3 g_par((a.m + FPL_CN_WAVES - 1) / FPL_CN_WAVES, tiles);
    const dim3 g_bit((a.n + 4 * FPL_BIT_RUN - 1) / (4 * FPL_BIT_RUN), tiles);
    hipLaunchKernelGGL(fpl_load_llr, g_llr, dim3(256), 0, s, a);
    hipLaunchKernelGGL(fpl_load_synd, g_m256, dim3(256), 0, s, a);
    for (int it = 0; it < a.max_it; ++it) {
        switch (a.alg) {
        case 0: launch_cn<0>(a, it, s); break;
        case 1: launch_cn<1>(a, it, s); break;
        case 2: launch_cn<2>(a, it, s); break;
        case 3: launch_cn<3>(a, it, s); break;
        case 4: launch_cn<4>(a, it, s); break;
        default: launch_cn<5>(a, it, s); break;
        }
        // adaptive: exit after this pass, iterations it + 1; the others: the pass's
        // head tested the decisions of iteration it - 1, iterations (it - 1) + 1
        if (adaptive || it > 0) hipLaunchKernelGGL(fpl_settle, dim3(tiles), dim3(64), 0, s, a, adaptive ? it + 1 : it, 1, 0);
        hipLaunchKernelGGL(fpl_bit, g_bit, dim3(256), 0, s, a);
        if (trace.unsat) {
            hipLaunchKernelGGL(fpl_trace_count, g_cnt, dim3(256), 0, s, a, trace);
            hipLaunchKernelGGL(fpl_trace_flush, dim3(tiles), dim3(64), 0, s, a, trace, it);
        }
        if (trace.post) hipLaunchKernelGGL(fpl_trace_post, g_llr, dim3(256), 0, s, a, trace, it);
    }
    if (!adaptive) hipLaunchKernelGGL(fpl_parity, g_par, dim3(64 * FPL_CN_WAVES), 0, s, a);
    hipLaunchKernelGGL(fpl_settle, dim3(tiles), dim3(64), 0, s, a, a.max_it, adaptive ? 0 : 1, 1);
    hipLaunchKernelGGL(fpl_store_bits, g_n256, dim3(256), 0, s, a);
    if (a.post) hipLaunchKernelGGL(fpl_store_post, g_llr, dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace qldpc
