// select.hip — the positions a symmetric blind round discloses (Kiktenko et al.,
// Phys. Rev. Applied 8, 044017, arXiv:1612.03673): for each listed frame the
// `count` candidate positions of smallest |posterior|.
//
// Order: position i sorts by the pair (u, i), u = the posterior's 64 bits with
// the sign cleared, compared as integers: +-0, denormals, normals, inf, NaN;
// equal magnitudes go to the lower index.  No floating-point compare is made.
// Candidates: every position that is neither shortened (cls[i] == 2) nor among
// the frame's earlier positions pos[f][0 .. first).
//
// One workgroup per listed frame.  The row (8 n bytes) stays in global memory
// and is read once per pass; LDS holds the excluded positions as a bit mask,
// one digit histogram and the winners.
//   1. MSB-first radix select on u: digits of 11, 11, 11, 11, 11 and 8 bits
//      (63 bits in all).  A pass histograms the digit of the candidates whose
//      higher digits equal the prefix found so far, and the bucket that holds
//      the k-th smallest extends the prefix.  The passes end as soon as that
//      bucket is taken whole (its size equals what is still to be taken): with
//      distinct magnitudes after 2-3 passes, with ties after all 6.
//   2. One collection pass in index order: keys whose decided digits are below
//      the prefix, and the first k of those that equal it (a workgroup scan of
//      ballots places them: nothing atomic, the same slots on every run).
//   3. A bitonic sort of the winners by (u, i) in LDS; plain vector stores of
//      the indices to pos[f][first .. first + count).
// A count beyond the candidates (the caller's contract) leaves -1 in the
// entries that no candidate fills; nothing is read or written out of bounds.
#include "decoder_common.hpp"

namespace qldpc {

namespace {

constexpr int DIGIT_BITS = 11, HIST_BINS = 1 << DIGIT_BITS, KEY_BITS = 63;
constexpr uint64_t MAG = 0x7fffffffffffffffull;

struct Bucket {  // what a pass found, written by the one thread that owns the bucket
    uint32_t found, digit, before, size;
};

// Exclusive prefix of v over the workgroup's threads in thread order, and the
// total.  wsum holds one word per wave; two barriers, so it can be used again.
__device__ inline uint32_t block_scan(uint32_t v, uint32_t *wsum, uint32_t &total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = (blockDim.x + 63) >> 6;
    uint32_t inc = v;
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(inc, d, 64);
        if (lane >= d) inc += o;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    uint32_t base = 0, t = 0;
    for (int w = 0; w < waves; ++w) {
        const uint32_t s = wsum[w];
        base += w < wave ? s : 0;
        t += s;
    }
    __syncthreads();
    total = t;
    return base + inc - v;
}

__device__ __forceinline__ bool pair_greater(uint64_t ua, int32_t ia, uint64_t ub, int32_t ib) {
    return ua > ub || (ua == ub && ia > ib);
}

// Dynamic LDS: keys[p2] (8 bytes each), idx[p2], hist[HIST_BINS], mask[(n + 31) / 32],
// wsum[16], one Bucket; p2 = the power of two >= count (select_lds).  blockDim.x
// is a multiple of 64.
__global__ void __launch_bounds__(1024) select_kernel(int n, int batch, const uint8_t *cls, const int32_t *list,
                                                     const double *post, int first, int count, int p2, int32_t *pos,
                                                     int cap) {
    extern __shared__ uint64_t lds[];
    const int nw = (n + 31) / 32;
    uint64_t *keys = lds;
    int32_t *idx = reinterpret_cast<int32_t *>(keys + p2);
    uint32_t *hist = reinterpret_cast<uint32_t *>(idx + p2);
    uint32_t *mask = hist + HIST_BINS;
    uint32_t *wsum = mask + nw;
    Bucket *bucket = reinterpret_cast<Bucket *>(wsum + 16);

    const size_t j = blockIdx.x, f = list ? (size_t)(uint32_t)list[j] : j;
    if (f >= (size_t)batch) return;  // (the caller's contract; the whole workgroup leaves)
    const uint64_t *row = reinterpret_cast<const uint64_t *>(post) + f * (size_t)n;
    int32_t *prow = pos + f * (size_t)cap;
    const int T = blockDim.x, tid = threadIdx.x;

    // the excluded positions: shortened ones and the tail of the last word, then the history
    for (int w = tid; w < nw; w += T) {
        uint32_t v = 0;
        for (int b = 0; b < 32; ++b) {
            const int i = 32 * w + b;
            if (i >= n || (cls && cls[i] == 2)) v |= 1u << b;
        }
        mask[w] = v;
    }
    for (int s = tid; s < p2; s += T) {
        keys[s] = ~0ull;  // above every key: the padding of the sort
        idx[s] = -1;
    }
    __syncthreads();
    for (int h = tid; h < first; h += T) {
        const int p = prow[h];
        if ((unsigned)p < (unsigned)n) atomicOr(&mask[p >> 5], 1u << (p & 31));
    }
    __syncthreads();
    auto key_of = [&](int i, uint64_t &u) -> bool {  // false: not a candidate
        if (i >= n || ((mask[i >> 5] >> (i & 31)) & 1u)) return false;
        u = row[i] & MAG;
        return true;
    };

    // 1. the threshold: `prefix` = the bits [hi, 63) of the k-th smallest key
    uint64_t prefix = 0;
    uint32_t k = (uint32_t)count;
    int hi = KEY_BITS;
    while (hi > 0) {
        const int bits = hi >= DIGIT_BITS ? DIGIT_BITS : hi;  // 63 = 5 * 11 + 8
        const int shift = hi - bits, bins = 1 << bits;
        for (int b = tid; b < bins; b += T) hist[b] = 0;
        if (tid == 0) bucket->found = 0;
        __syncthreads();
        for (int i = tid; i < n; i += T) {
            uint64_t u;
            if (key_of(i, u) && (u >> hi) == prefix) atomicAdd(&hist[(uint32_t)(u >> shift) & (uint32_t)(bins - 1)], 1u);
        }
        __syncthreads();
        // thread t owns the bins [t * per, (t + 1) * per): the one whose range holds the k-th names the bucket
        const int per = bins > T ? bins / T : 1;
        uint32_t own = 0;
        if (tid * per < bins)
            for (int b = 0; b < per; ++b) own += hist[tid * per + b];
        uint32_t total;
        uint32_t before = block_scan(own, wsum, total);
        if (tid * per < bins && before < k && k <= before + own) {
            for (int b = 0; b < per; ++b) {
                const uint32_t c = hist[tid * per + b];
                if (k <= before + c) {
                    *bucket = Bucket{1u, (uint32_t)(tid * per + b), before, c};
                    break;
                }
                before += c;
            }
        }
        __syncthreads();
        const Bucket bk = *bucket;
        __syncthreads();  // (read by all before the next pass clears it)
        if (!bk.found) break;  // fewer candidates than count: everything is taken (hi == 63, prefix == 0)
        prefix = (prefix << bits) | bk.digit;
        k -= bk.before;
        hi = shift;
        if (bk.size == k) break;  // the bucket is taken whole: the lower digits decide nothing
    }

    // 2. the winners, in index order: decided bits below the prefix, and the first k that equal it
    const uint32_t n_less = (uint32_t)count - k;
    uint32_t less_seen = 0, eq_seen = 0;
    for (int base = 0; base < n; base += T) {
        uint64_t u = 0;
        const bool cand = key_of(base + tid, u);
        const uint64_t d = u >> hi;
        const bool lt = cand && d < prefix, eq = cand && d == prefix;
        uint32_t total;
        const uint32_t ex = block_scan((lt ? 1u : 0u) | (eq ? 1u << 16 : 0u), wsum, total);  // (T <= 1024 < 2^16)
        const uint32_t slot = lt ? less_seen + (ex & 0xffffu) : n_less + eq_seen + (ex >> 16);
        if ((lt || (eq && eq_seen + (ex >> 16) < k)) && slot < (uint32_t)count) {
            keys[slot] = u;
            idx[slot] = base + tid;
        }
        less_seen += total & 0xffffu;
        eq_seen += total >> 16;
    }
    __syncthreads();

    // 3. sort by (u, i); the padding (and what a short row left unfilled) ends up last
    for (int k2 = 2; k2 <= p2; k2 <<= 1) {
        for (int s = k2 >> 1; s > 0; s >>= 1) {
            for (int t = tid; t < p2 / 2; t += T) {
                const int a = ((t & ~(s - 1)) << 1) | (t & (s - 1)), b = a | s;
                const uint64_t ua = keys[a], ub = keys[b];
                const int32_t ia = idx[a], ib = idx[b];
                const bool up = (a & k2) == 0;
                if (pair_greater(ua, ia, ub, ib) == up) {
                    keys[a] = ub; keys[b] = ua;
                    idx[a] = ib; idx[b] = ia;
                }
            }
            __syncthreads();
        }
    }
    for (int r = tid; r < count; r += T) prow[first + r] = idx[r];
}

int pow2_at_least(int v) {
    int p = 1;
    while (p < v) p <<= 1;
    return p;
}

}  // namespace

size_t select_lds(int n, int count) {
    const size_t p2 = (size_t)pow2_at_least(count);
    return p2 * (sizeof(uint64_t) + sizeof(int32_t)) +
           ((size_t)HIST_BINS + (size_t)((n + 31) / 32) + 16) * sizeof(uint32_t) + sizeof(Bucket);
}

hipError_t launch_select(int n, int batch, const uint8_t *cls, int n_list, const int32_t *list, const double *post,
                         int first, int count, int32_t *pos, int cap, hipStream_t stream) {
    if (n_list <= 0 || count <= 0) return hipSuccess;
    if (count > SELECT_MAX || first < 0 || (long long)first + count > cap) return hipErrorInvalidValue;
    const size_t lds = select_lds(n, count);
    if (lds > LDS_MAX_BYTES) return hipErrorInvalidValue;
    if (lds > 65536) {
        const hipError_t e = allow_dynamic_lds(reinterpret_cast<const void *>(select_kernel), lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(select_kernel, dim3(n_list), dim3(aux_frame_threads(n)), lds, stream, n, batch, cls, list, post,
                       first, count, pow2_at_least(count), pos, cap);
    return hipGetLastError();
}

}  // namespace qldpc
