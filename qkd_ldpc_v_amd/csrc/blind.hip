// blind.hip — the disclosure rounds of blind reconciliation (Martinez-Mateo,
// Elkouss, Martin, arXiv:1205.5729) around the per-party cut of parties.hip.
//
// A frame whose decode failed (syndromes_match == 0) is decoded again after
// Alice has disclosed the values of some of her punctured bits: Bob pins those
// positions at +-DBL_MAX and keeps everything else of the frame.  Between
// rounds only the list of failed frames and the disclosed bits cross the
// channel:
//   - failed_frames_kernel: the indices of the frames with synd_ok == 0,
//     ascending, and their count;
//   - disclose_kernel (Alice): her fill at the disclosed punctured indices, for
//     the listed frames;
//   - round_frames_kernel (Bob): compact row j of the round's LLRs and
//     syndromes, for frame list[j] — what bob_frames_kernel writes for that
//     frame, with the disclosed positions pinned;
//   - scatter_kernel: the compact decode results back to rows list[j].
// A symmetric round (arXiv:1612.03673) discloses per-frame positions instead,
// the ones select.hip picked from Bob's posteriors:
//   - disclose_positions_kernel (Alice): her bits at the frame's new positions;
//   - positions_frames_kernel (Bob): round_frames_kernel with the frame's own
//     position history pinned, of any class, with or without a plan.
// One workgroup per listed frame where a frame is the unit.  Every global store
// is a plain vector store.
#include "decoder_common.hpp"

namespace qldpc {

namespace {

constexpr int LIST_THREADS = 1024;  // frames per workgroup of failed_frames_kernel
constexpr double PIN = 1.7976931348623157e308;  // DBL_MAX

// bytes of p[0, len) that are 0, summed over the workgroup's threads by the caller
__device__ inline uint32_t zero_bytes_strided(const uint8_t *p, size_t len) {
    // 8-byte words between the first aligned address and the end; the bytes around them one by one
    const size_t to_aligned = (8 - (reinterpret_cast<uintptr_t>(p) & 7)) & 7, head = len < to_aligned ? len : to_aligned;
    const size_t words = (len - head) / 8, tail0 = head + 8 * words;
    uint32_t c = 0;
    const uint64_t *w = reinterpret_cast<const uint64_t *>(p + head);
    for (size_t i = threadIdx.x; i < words; i += blockDim.x) {
        uint64_t x = w[i];  // a byte's bits folded into its bit 0
        x |= x >> 4;
        x |= x >> 2;
        x |= x >> 1;
        c += 8 - (uint32_t)__popcll(x & 0x0101010101010101ull);
    }
    for (size_t i = threadIdx.x; i < head; i += blockDim.x) c += p[i] == 0;
    for (size_t i = tail0 + threadIdx.x; i < len; i += blockDim.x) c += p[i] == 0;
    return c;
}

// Workgroup b places the failed frames of [b * 1024, (b + 1) * 1024): its base
// is the count of failed frames before them, which it takes from synd_ok
// itself (wide loads; no scratch, no second launch, nothing atomic), then a
// ballot per wave and a scan of the wave counts give every frame its place.
// The order is ascending whatever the schedule.
__global__ void __launch_bounds__(LIST_THREADS) failed_frames_kernel(int batch, const uint8_t *synd_ok,
                                                                     int32_t *list, int32_t *count) {
    __shared__ uint32_t wsum[LIST_THREADS / 64];
    __shared__ uint32_t base_s;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t first = (size_t)blockIdx.x * LIST_THREADS;

    uint32_t c = zero_bytes_strided(synd_ok, first);
    for (int d = 32; d > 0; d >>= 1) c += __shfl_xor(c, d, 64);
    if (lane == 0) wsum[wave] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t s = 0;
        for (int w = 0; w < LIST_THREADS / 64; ++w) s += wsum[w];
        base_s = s;
    }
    __syncthreads();
    const uint32_t base = base_s;

    const size_t i = first + threadIdx.x;
    const bool failed = i < (size_t)batch && synd_ok[i] == 0;
    const uint64_t bal = __ballot(failed);
    if (lane == 0) wsum[wave] = (uint32_t)__popcll(bal);  // (the base's wave sums were read before the last barrier)
    __syncthreads();
    uint32_t before = 0, total = 0;
    for (int w = 0; w < LIST_THREADS / 64; ++w) {
        before += w < wave ? wsum[w] : 0;
        total += wsum[w];
    }
    if (failed) list[base + before + (uint32_t)__popcll(bal & ((1ull << lane) - 1))] = (int32_t)i;
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) *count = (int32_t)(base + total);
}

// out[j][i] = fill[list[j]][disc[i]]; list == NULL: frame j.  An index outside
// the plan's punctured list (the caller's contract) reads nothing and writes 0.
__global__ void __launch_bounds__(256) disclose_kernel(int n_punct, const int32_t *list, const uint8_t *fill,
                                                       int n_disc, const int32_t *disc, uint8_t *out) {
    const size_t j = blockIdx.x, f = list ? (size_t)list[j] : j;
    const uint8_t *row = fill + f * (size_t)n_punct;
    uint8_t *o = out + j * (size_t)n_disc;
    for (int i = threadIdx.x; i < n_disc; i += blockDim.x) {
        const int k = disc[i];
        o[i] = (unsigned)k < (unsigned)n_punct ? row[k] : (uint8_t)0;
    }
}

// Compact row j of the round: frame f = list[j] (list == NULL: f = j).  Bob's
// key as bit words and one byte per punctured index k (0: not disclosed, 1 / 2:
// disclosed 0 / 1) live in LDS, so position i takes its value from cls[i] /
// src[i] alone and the LLR stores run along i: bob_frames_kernel's values, and
// +-DBL_MAX (the builder's sign, bit ? -lp : lp) where k = src[i] is disclosed.
__global__ void __launch_bounds__(1024) round_frames_kernel(int n, int m, int batch, int n_punct, const uint8_t *cls,
                                                           const int32_t *src, const int32_t *list,
                                                           const uint8_t *key, const double *log_p,
                                                           const uint8_t *synd, int n_disc, const int32_t *disc,
                                                           const uint8_t *vals, double *llr, uint8_t *synd_ws) {
    extern __shared__ uint32_t kb[];
    const int nw = (n + 31) / 32;
    uint32_t *bbits = kb;
    uint8_t *dtab = reinterpret_cast<uint8_t *>(kb + nw);
    const size_t j = blockIdx.x, f = list ? (size_t)(uint32_t)list[j] : j;
    if (f >= (size_t)batch) return;  // (the caller's contract; the whole workgroup leaves)
    const double lp = log_p[f];
    dev::pack_key_bits(key + f * (size_t)n, n, bbits);
    for (int k = threadIdx.x; k < n_punct; k += blockDim.x) dtab[k] = 0;
    __syncthreads();
    for (int i = threadIdx.x; i < n_disc; i += blockDim.x) {
        const int k = disc[i];
        if ((unsigned)k < (unsigned)n_punct) dtab[k] = (uint8_t)(1 + (vals[j * (size_t)n_disc + i] & 1u));
    }
    __syncthreads();
    double *l = llr + j * (size_t)n;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const int c = cls[i];
        double v;
        if (c == 0) {
            v = dev::key_bit(bbits, src[i]) ? -lp : lp;
        } else if (c == 1) {
            const int d = dtab[src[i]];
            v = d == 0 ? 1e-4 : d == 1 ? PIN : -PIN;
        } else {
            v = PIN;
        }
        l[i] = v;
    }
    const uint8_t *s = synd + f * (size_t)m;
    uint8_t *sw = synd_ws + j * (size_t)m;
    for (int r = threadIdx.x; r < m; r += blockDim.x) sw[r] = s[r];
}

// Symmetric rounds (select.hip picks the positions): Alice's answer for the
// positions pos[f][first .. first + count) of frame f = list[j] (NULL: f = j),
// out[j][i] = ext[f][pos[f][first + i]] & 1.  A position outside [0, n) (the
// caller's contract) reads nothing and writes 0.
__global__ void __launch_bounds__(256) disclose_positions_kernel(int n, const int32_t *list, const uint8_t *ext,
                                                                 size_t ext_stride, const int32_t *pos, int cap,
                                                                 int first, int count, uint8_t *out) {
    const size_t j = blockIdx.x, f = list ? (size_t)(uint32_t)list[j] : j;
    const uint8_t *row = ext + f * ext_stride;
    const int32_t *p = pos + f * (size_t)cap + first;
    uint8_t *o = out + j * (size_t)count;
    for (int i = threadIdx.x; i < count; i += blockDim.x) {
        const int k = p[i];
        o[i] = (unsigned)k < (unsigned)n ? (uint8_t)(row[k] & 1u) : (uint8_t)0;
    }
}

// round_frames_kernel for a positions round: bob_frames_kernel's values for
// frame f = list[j] (NULL: f = j), then position pos[f][i] pinned at
// vals[j][i] ? -DBL_MAX : +DBL_MAX for i < n_disc, whatever its class.  cls ==
// NULL: no plan.  LDS: Bob's key, the pinned positions and their bits, one bit
// word array each.
__global__ void __launch_bounds__(1024) positions_frames_kernel(int n, int m, int batch, const uint8_t *cls,
                                                               const int32_t *src, const int32_t *list,
                                                               const uint8_t *key, const double *log_p,
                                                               const uint8_t *synd, int n_disc, const int32_t *pos,
                                                               int cap, const uint8_t *vals, double *llr,
                                                               uint8_t *synd_ws) {
    extern __shared__ uint32_t kb[];
    const int nw = (n + 31) / 32;
    uint32_t *bbits = kb, *pinned = kb + nw, *pinbit = kb + 2 * nw;
    const size_t j = blockIdx.x, f = list ? (size_t)(uint32_t)list[j] : j;
    if (f >= (size_t)batch) return;  // (the caller's contract; the whole workgroup leaves)
    const double lp = log_p[f];
    dev::pack_key_bits(key + f * (size_t)n, n, bbits);
    for (int w = threadIdx.x; w < 2 * nw; w += blockDim.x) pinned[w] = 0;
    __syncthreads();
    const int32_t *p = pos + f * (size_t)cap;
    for (int i = threadIdx.x; i < n_disc; i += blockDim.x) {
        const int k = p[i];
        if ((unsigned)k < (unsigned)n) {
            atomicOr(&pinned[k >> 5], 1u << (k & 31));
            if (vals[j * (size_t)n_disc + i] & 1u) atomicOr(&pinbit[k >> 5], 1u << (k & 31));
        }
    }
    __syncthreads();
    double *l = llr + j * (size_t)n;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const int c = cls ? cls[i] : 0;
        double v;
        if (dev::key_bit(pinned, i)) v = dev::key_bit(pinbit, i) ? -PIN : PIN;
        else if (c == 0) v = dev::key_bit(bbits, cls ? src[i] : i) ? -lp : lp;
        else v = c == 1 ? 1e-4 : PIN;
        l[i] = v;
    }
    const uint8_t *s = synd + f * (size_t)m;
    uint8_t *sw = synd_ws + j * (size_t)m;
    for (int r = threadIdx.x; r < m; r += blockDim.x) sw[r] = s[r];
}

// Rows list[j] of the caller's arrays <- compact row j of the round's decode.
__global__ void __launch_bounds__(1024) scatter_kernel(int n, int batch, const int32_t *list, const uint8_t *cbits,
                                                      const uint32_t *citers, const uint8_t *cok, const double *cpost,
                                                      uint8_t *bits, uint32_t *iters, uint8_t *ok, double *post) {
    const size_t j = blockIdx.x, f = (size_t)(uint32_t)list[j];
    if (f >= (size_t)batch) return;
    const uint8_t *cb = cbits + j * (size_t)n;
    uint8_t *b = bits + f * (size_t)n;
    for (int i = threadIdx.x; i < n; i += blockDim.x) b[i] = cb[i];
    if (post) {
        const double *cp = cpost + j * (size_t)n;
        double *p = post + f * (size_t)n;
        for (int i = threadIdx.x; i < n; i += blockDim.x) p[i] = cp[i];
    }
    if (threadIdx.x == 0) {
        iters[f] = citers[j];
        ok[f] = cok[j];
    }
}

}  // namespace

hipError_t launch_failed_frames(int batch, const uint8_t *synd_ok, int32_t *list, int32_t *count,
                                hipStream_t stream) {
    if (batch <= 0) return hipSuccess;
    const int blocks = (int)(((long long)batch + LIST_THREADS - 1) / LIST_THREADS);
    hipLaunchKernelGGL(failed_frames_kernel, dim3(blocks), dim3(LIST_THREADS), 0, stream, batch, synd_ok, list, count);
    return hipGetLastError();
}

hipError_t launch_disclose(int n_punct, int n_list, const int32_t *list, const uint8_t *fill, int n_disc,
                           const int32_t *disc, uint8_t *out, hipStream_t stream) {
    if (n_list <= 0 || n_disc <= 0) return hipSuccess;
    hipLaunchKernelGGL(disclose_kernel, dim3(n_list), dim3(256), 0, stream, n_punct, list, fill, n_disc, disc, out);
    return hipGetLastError();
}

hipError_t launch_round_frames(int n, int m, int batch, int n_punct, const uint8_t *cls, const int32_t *src,
                               int n_list, const int32_t *list, const uint8_t *key, const double *log_p,
                               const uint8_t *synd, int n_disc, const int32_t *disc, const uint8_t *vals,
                               double *llr, uint8_t *synd_ws, hipStream_t stream) {
    if (n_list <= 0) return hipSuccess;
    const size_t lds = round_frames_lds(n, n_punct);
    if (lds > LDS_MAX_BYTES) return hipErrorInvalidValue;
    if (lds > 65536) {
        const hipError_t e = allow_dynamic_lds(reinterpret_cast<const void *>(round_frames_kernel), lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(round_frames_kernel, dim3(n_list), dim3(aux_frame_threads(n)), lds, stream, n, m, batch,
                       n_punct, cls, src, list, key, log_p, synd, n_disc, disc, vals, llr, synd_ws);
    return hipGetLastError();
}

hipError_t launch_disclose_positions(int n, int n_list, const int32_t *list, const uint8_t *ext, size_t ext_stride,
                                     const int32_t *pos, int cap, int first, int count, uint8_t *out,
                                     hipStream_t stream) {
    if (n_list <= 0 || count <= 0) return hipSuccess;
    if (first < 0 || (long long)first + count > cap) return hipErrorInvalidValue;
    hipLaunchKernelGGL(disclose_positions_kernel, dim3(n_list), dim3(256), 0, stream, n, list, ext, ext_stride, pos, cap,
                       first, count, out);
    return hipGetLastError();
}

hipError_t launch_positions_frames(int n, int m, int batch, const uint8_t *cls, const int32_t *src, int n_list,
                                   const int32_t *list, const uint8_t *key, const double *log_p, const uint8_t *synd,
                                   int n_disc, const int32_t *pos, int cap, const uint8_t *vals, double *llr,
                                   uint8_t *synd_ws, hipStream_t stream) {
    if (n_list <= 0) return hipSuccess;
    if (n_disc < 0 || n_disc > cap) return hipErrorInvalidValue;
    const size_t lds = positions_frames_lds(n);
    if (lds > LDS_MAX_BYTES) return hipErrorInvalidValue;
    if (lds > 65536) {
        const hipError_t e = allow_dynamic_lds(reinterpret_cast<const void *>(positions_frames_kernel), lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(positions_frames_kernel, dim3(n_list), dim3(aux_frame_threads(n)), lds, stream, n, m, batch, cls,
                       src, list, key, log_p, synd, n_disc, pos, cap, vals, llr, synd_ws);
    return hipGetLastError();
}

hipError_t launch_round_scatter(int n, int batch, int n_list, const int32_t *list, const uint8_t *cbits,
                                const uint32_t *citers, const uint8_t *cok, const double *cpost, uint8_t *bits,
                                uint32_t *iters, uint8_t *ok, double *post, hipStream_t stream) {
    if (n_list <= 0) return hipSuccess;
    hipLaunchKernelGGL(scatter_kernel, dim3(n_list), dim3(aux_frame_threads(n)), 0, stream, n, batch, list, cbits,
                       citers, cok, cpost, bits, iters, ok, post);
    return hipGetLastError();
}

}  // namespace qldpc
