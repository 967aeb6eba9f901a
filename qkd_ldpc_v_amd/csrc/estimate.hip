// estimate.hip — the QBER at the reconciliation stage (Kiktenko et al.,
// arXiv:1810.05841), from data the exchange already holds.
//   - before the decode: Bob's own syndrome against the one he received.  The
//     weight of their difference over the informative rows is a sufficient
//     statistic for q: syndrome_weight_kernel; solve_kernel turns each weight
//     into q and log_p (estimate_math.h, the function the host entry calls);
//   - after the decode: the positions where Bob's key differs from the decoded
//     frame, the frame's error count: corrected_errors_kernel.
// One workgroup per frame, as in parties.hip; the solve takes one thread per
// frame (about 2,000 dependent f64 operations each: lanes stay full, the
// syndrome workgroups never wait on one lane).  Key bytes are 0 or 1: only
// bit 0 is read.  Every global store is a plain vector store.
#include "decoder_common.hpp"
#include "estimate_math.h"

namespace qldpc {

namespace {

// row_d[j]: the effective degree of row j when it is informative, else 0
// (capi.hip est_row_table; without a plan it is row_deg itself).  cls == NULL:
// no plan, the extended key is the key.  With a plan position i of the
// extended key is key[src[i]] (cls 0) or 0 (punctured and shortened: Bob holds
// nothing there, and rows with a punctured neighbour are not counted).
__global__ void __launch_bounds__(1024) syndrome_weight_kernel(int n, int m, const int32_t *ell_col,
                                                              const int32_t *row_deg, const int32_t *row_d,
                                                              const uint8_t *cls, const int32_t *src,
                                                              const uint8_t *key, const uint8_t *synd,
                                                              int32_t *weight) {
    extern __shared__ uint32_t kb[];
    __shared__ int total;
    const int nw = (n + 31) / 32, xw = 2 * ((n + 63) / 64);
    uint32_t *bbits = kb, *xbits = cls ? kb + nw : kb;
    const size_t f = blockIdx.x;
    const int lane = threadIdx.x & 63;
    if (threadIdx.x == 0) total = 0;
    dev::pack_key_bits(key + f * (size_t)n, n, bbits);
    __syncthreads();
    if (cls) {
        // the extended key, 64 positions per wave ballot
        for (int base = (int)(threadIdx.x & ~63u); base < 32 * xw; base += blockDim.x) {
            const int i = base + lane;
            const uint32_t bit = (i < n && cls[i] == 0) ? dev::key_bit(bbits, src[i]) : 0u;
            const uint64_t bal = __ballot(bit);
            if (lane == 0) {
                xbits[base >> 5] = (uint32_t)bal;
                xbits[(base >> 5) + 1] = (uint32_t)(bal >> 32);
            }
        }
        __syncthreads();
    }
    const uint8_t *s = synd + f * (size_t)m;
    int count = 0;  // (wave-uniform: a ballot's population)
    for (int base = (int)(threadIdx.x & ~63u); base < m; base += blockDim.x) {
        const int j = base + lane;
        uint32_t z = 0;
        if (j < m) {
            // the table entry and the syndrome byte are requested beside the row's
            // columns, not ahead of them: a workgroup's time is its chain of
            // dependent loads (testing row_d before the row is read: 72 us per
            // 4096 C2 frames instead of 65; DESIGN.md "The estimator")
            const int d = row_d[j];
            const uint32_t sj = s[j];
            const uint32_t p = dev::row_parity(xbits, ell_col, row_deg, m, j);
            z = d > 0 ? (p ^ sj) & 1u : 0u;
        }
        count += __popcll(__ballot(z));
    }
    if (lane == 0) atomicAdd(&total, count);
    __syncthreads();
    if (threadIdx.x == 0) weight[f] = total;
}

// The class table travels as a kernel argument: a few dozen entries at most.
struct ClassArg {
    int32_t count;
    int32_t degree[EST_MAX_CLASSES], rows[EST_MAX_CLASSES];
};

__global__ void __launch_bounds__(64) solve_kernel(int batch, ClassArg ca, const int32_t *weight, double q_min,
                                                  double q_max, double *qber, double *log_p) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= batch) return;
    const ql_exact::EstClasses cl = {ca.count, ca.degree, ca.rows};
    const double q = ql_exact::est_qber(cl, (int64_t)weight[f], 1, q_min, q_max);
    if (qber) qber[f] = q;
    if (log_p) log_p[f] = ql_exact::est_log_p(q);
}

__device__ __forceinline__ int diff4(uint32_t a, uint32_t b) { return __popc((a ^ b) & 0x01010101u); }

// cls == NULL: the Hamming distance of two n-byte rows (bit 0 of each byte),
// 16 bytes per load where both rows are 16-byte aligned.  With a plan only key
// positions count: key[src[i]] against bits[i] where cls[i] == 0, four
// positions per step where the bits row is 4-byte aligned (cls and src are
// allocations of their own: aligned).
__global__ void __launch_bounds__(1024) corrected_errors_kernel(int n, const uint8_t *cls, const int32_t *src,
                                                               const uint8_t *key, const uint8_t *bits,
                                                               int32_t *errors) {
    __shared__ int total;
    const size_t f = blockIdx.x;
    const uint8_t *k = key + f * (size_t)n, *b = bits + f * (size_t)n;
    if (threadIdx.x == 0) total = 0;
    __syncthreads();
    int count = 0, done = 0;  // positions [0, done) are counted by the wide loop
    if (!cls) {
        if (((reinterpret_cast<uintptr_t>(k) | reinterpret_cast<uintptr_t>(b)) & 15) == 0) {
            const uint4 *k4 = reinterpret_cast<const uint4 *>(k), *b4 = reinterpret_cast<const uint4 *>(b);
            for (int v = threadIdx.x; v < n / 16; v += blockDim.x) {
                const uint4 x = k4[v], y = b4[v];
                count += diff4(x.x, y.x) + diff4(x.y, y.y) + diff4(x.z, y.z) + diff4(x.w, y.w);
            }
            done = n / 16 * 16;
        }
        for (int i = done + threadIdx.x; i < n; i += blockDim.x) count += (k[i] ^ b[i]) & 1;
    } else {
        if ((reinterpret_cast<uintptr_t>(b) & 3) == 0) {
            const uint32_t *c4 = reinterpret_cast<const uint32_t *>(cls), *b4 = reinterpret_cast<const uint32_t *>(b);
            const int4 *s4 = reinterpret_cast<const int4 *>(src);
            for (int v = threadIdx.x; v < n / 4; v += blockDim.x) {
                const uint32_t c = c4[v], y = b4[v];
                const int4 s = s4[v];
                if ((c & 0xffu) == 0) count += (k[s.x] ^ y) & 1;
                if ((c & 0xff00u) == 0) count += (k[s.y] ^ (y >> 8)) & 1;
                if ((c & 0xff0000u) == 0) count += (k[s.z] ^ (y >> 16)) & 1;
                if ((c & 0xff000000u) == 0) count += (k[s.w] ^ (y >> 24)) & 1;
            }
            done = n / 4 * 4;
        }
        for (int i = done + threadIdx.x; i < n; i += blockDim.x)
            if (cls[i] == 0) count += (k[src[i]] ^ b[i]) & 1;
    }
    for (int o = 32; o > 0; o >>= 1) count += __shfl_down(count, o, 64);
    if ((threadIdx.x & 63) == 0) atomicAdd(&total, count);
    __syncthreads();
    if (threadIdx.x == 0) errors[f] = total;
}

}  // namespace

hipError_t launch_syndrome_weight(int n, int m, const int32_t *ell_col, const int32_t *row_deg, const int32_t *row_d,
                                  const uint8_t *cls, const int32_t *src, int batch, const uint8_t *key,
                                  const uint8_t *synd, int32_t *weight, hipStream_t stream) {
    if (batch <= 0) return hipSuccess;
    const size_t lds = syndrome_weight_lds(n, cls != nullptr);
    if (lds > LDS_MAX_BYTES) return hipErrorInvalidValue;
    if (lds > 65536) {
        const hipError_t e = allow_dynamic_lds(reinterpret_cast<const void *>(syndrome_weight_kernel), lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(syndrome_weight_kernel, dim3(batch), dim3(aux_frame_threads(n)), lds, stream, n, m, ell_col,
                       row_deg, row_d, cls, src, key, synd, weight);
    return hipGetLastError();
}

hipError_t launch_estimate_solve(int batch, int n_classes, const int32_t *degree, const int32_t *rows,
                                 const int32_t *weight, double q_min, double q_max, double *qber, double *log_p,
                                 hipStream_t stream) {
    if (batch <= 0) return hipSuccess;
    if (n_classes < 1 || n_classes > EST_MAX_CLASSES) return hipErrorInvalidValue;
    ClassArg ca = {};
    ca.count = n_classes;
    for (int c = 0; c < n_classes; ++c) {
        ca.degree[c] = degree[c];
        ca.rows[c] = rows[c];
    }
    hipLaunchKernelGGL(solve_kernel, dim3((batch + 63) / 64), dim3(64), 0, stream, batch, ca, weight, q_min, q_max, qber,
                       log_p);
    return hipGetLastError();
}

hipError_t launch_corrected_errors(int n, const uint8_t *cls, const int32_t *src, int batch, const uint8_t *key,
                                   const uint8_t *bits, int32_t *errors, hipStream_t stream) {
    if (batch <= 0) return hipSuccess;
    hipLaunchKernelGGL(corrected_errors_kernel, dim3(batch), dim3(aux_frame_threads(n)), 0, stream, n, cls, src, key,
                       bits, errors);
    return hipGetLastError();
}

}  // namespace qldpc
