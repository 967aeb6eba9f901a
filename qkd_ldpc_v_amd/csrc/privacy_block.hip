// privacy_block.hip — the Toeplitz hash of one long block: the concatenation of
// a list of frames' keys, hashed as a whole in O(N log N).
//
// With the block x[0..L), the seed s[0..L+r-1) and r outputs, the header's
//     y[i] = XOR over j in [0, L) of  s[i + L - 1 - j] & x[j]
// is bit 0 of (s * x)[i + L - 1], `*` the linear convolution over the integers.
// In the cyclic convolution of length N = 2^k >= L + r - 1 the wrapped terms
// land on indices <= L - 2 only, so indices L - 1 .. L + r - 2 are exact, and a
// coefficient is a count <= L <= 2^27 < p: a number-theoretic transform modulo
// the one prime p = 15 * 2^27 + 1 (primitive root 31) recovers it exactly.
//
// Layout of the transform.  Forward: decimation in frequency (natural order in,
// bit-reversed out); back: decimation in time (bit-reversed in, natural out),
// so no pass reorders anything.  The backward transform runs with the FORWARD
// roots: it returns N conv[(N - n) mod N] at index n, the extraction reads
// index (N - (L - 1 + i)) mod N, and the one table serves both directions.  The
// lowest min(k, 12) stages run on a contiguous tile of 4096 points in LDS (the
// tile pass); the stages above it run as strided passes of at most
// NTT_PASS_STAGES stages: a workgroup loads 2^c rows, 2^(ls - c) points apart,
// of 4096 / 2^c consecutive points — a set closed under the c stages of half
// sizes 2^(ls - 1) .. 2^(ls - c) — into the same LDS tile.  The seed's tile
// pass, the pointwise product with the keys' spectrum, the 1/N scale and the
// first backward pass are one kernel (MODE_MID).
//
// Twiddles: W[m + j] = w_2m^j (j < m, m a power of two; w_2m = w_N^(N / 2m)),
// N entries in the workspace, built at the head of every call.  A stage of half
// size m reads W[m ..2m) in the order of its points, so the strided passes read
// it coalesced and the tile pass keeps W[0 .. 4096) in LDS.
//
// Ranges (P = p, R = 2^32; 2P < R since P < 2^31).  Points are plain residues in
// [0, P) between stages; table entries are Montgomery forms w R mod P in [0, P).
//   montmul(a, b), a < R, b < P:  T = a b < R P.  m = lo(T) P^-1 mod R makes
//     lo(m P) = lo(T), so (T - m P) / R = hi(T) - hi(m P) without a borrow from
//     the low words; hi(T) < P and hi(m P) < P, so d = hi(T) - hi(m P) lies in
//     (-P, P).  As unsigned, d >= 0 gives d < P <= d + P; d < 0 wraps to
//     >= R - P + 1 > P > d + P (mod R).  min(d, d + P) is the residue in [0, P).
//   DIF butterfly, a, b in [0, P):  a + b < 2P < R, and min(s, s - P) reduces it
//     (s < P: s - P wraps above s).  a - b + P lies in (0, 2P) and goes into
//     montmul UNREDUCED as its first argument (< R): this is the lazy step.
//   DIT butterfly, a in [0, P), t = montmul(b, w) in [0, P):  a + t as above;
//     a - t in (-P, P), min(d, d + P) as in montmul.
//   Pointwise: montmul(montmul(x, y), K) with x, y, K < P and K = N^-1 R^2 mod P
//     is x y / N.
// Every global store is a plain vector store.
#include "decoder_common.hpp"

namespace qldpc {

namespace {

constexpr uint32_t NTT_P = 2013265921u;  // 15 * 2^27 + 1
constexpr uint32_t NTT_ROOT = 31;        // a primitive root of NTT_P
constexpr uint32_t ntt_pinv() {          // P^-1 mod 2^32 (Newton: each step doubles the correct low bits, from 3)
    uint32_t x = NTT_P;
    for (int i = 0; i < 5; ++i) x *= 2u - NTT_P * x;
    return x;
}
constexpr uint32_t NTT_PINV = ntt_pinv();
static_assert(NTT_PINV * NTT_P == 1u, "P^-1 mod 2^32");
constexpr int NTT_THREADS = 256;
constexpr int NTT_TILE = 1 << NTT_TILE_LOG;

// a b / R mod P for a < R, b < P (ranges: the head of the file)
__host__ __device__ inline uint32_t montmul(uint32_t a, uint32_t b) {
    const uint64_t t = (uint64_t)a * b;
    const uint32_t m = (uint32_t)t * NTT_PINV;
    const uint32_t d = (uint32_t)(t >> 32) - (uint32_t)(((uint64_t)m * NTT_P) >> 32);
    const uint32_t e = d + NTT_P;
    return d < e ? d : e;
}
__device__ __forceinline__ uint32_t add_mod(uint32_t a, uint32_t b) {
    const uint32_t s = a + b, e = s - NTT_P;
    return s < e ? s : e;
}
__device__ __forceinline__ uint32_t sub_mod(uint32_t a, uint32_t b) {
    const uint32_t d = a - b, e = d + NTT_P;
    return d < e ? d : e;
}

// w_N^(2^b) for b < 27 and 1, as Montgomery forms
struct NttRoots {
    uint32_t pw[27];
    uint32_t one;
};

__device__ __forceinline__ uint32_t root_power(const NttRoots &r, uint32_t e) {
    uint32_t v = r.one;
#pragma unroll
    for (int b = 0; b < 27; ++b)
        if ((e >> b) & 1u) v = montmul(v, r.pw[b]);
    return v;
}

// W[m + j] = w_N^(j N / 2m) for m = 2^lm < N, j < m.  2^lg threads: thread i takes j = i, i + 2^lg, ... of
// every level, the first by its power and each next one by a multiplication with w_2m^(2^lg).
__global__ void __launch_bounds__(NTT_THREADS) block_twiddles_kernel(uint32_t *W, int k, int lg, NttRoots r) {
    const uint32_t i = blockIdx.x * NTT_THREADS + threadIdx.x, G = 1u << lg;
    if (i == 0) W[0] = r.one;  // (never read by a stage)
    for (int lm = 0; lm < k; ++lm) {
        const uint32_t m = 1u << lm;
        const int sh = k - 1 - lm;
        if (i >= m) continue;
        uint32_t v = root_power(r, i << sh), step = 0;
#pragma unroll
        for (int b = 0; b < 27; ++b)
            if (b == lg + sh) step = r.pw[b];  // (read only where m > G: lg + sh <= k - 2)
        for (uint32_t j = i; j < m; j += G) {
            W[m + j] = v;
            v = montmul(v, step);
        }
    }
}

// A[i] = bit 0 of the block's entry i (0 past L), B[i] = bit 0 of the seed's entry i (0 past its S entries)
__global__ void __launch_bounds__(NTT_THREADS) block_pack_kernel(uint32_t N, uint32_t L, uint32_t S, uint32_t key_len,
                                                                long long key_stride, const int32_t *list,
                                                                const uint8_t *keys, const uint8_t *seed, uint32_t *A,
                                                                uint32_t *B) {
    const uint32_t i = blockIdx.x * NTT_THREADS + threadIdx.x;
    if (i >= N) return;
    uint32_t a = 0;
    if (i < L) {
        const uint32_t t = i / key_len, j = i - t * key_len;
        const size_t f = list ? (size_t)list[t] : (size_t)t;
        a = keys[f * (size_t)key_stride + j] & 1u;
    }
    A[i] = a;
    B[i] = i < S ? (seed[i] & 1u) : 0u;
}

__global__ void __launch_bounds__(NTT_THREADS) block_extract_kernel(uint32_t N, uint32_t L, uint32_t r,
                                                                   const uint32_t *B, uint8_t *out) {
    const uint32_t i = blockIdx.x * NTT_THREADS + threadIdx.x;
    if (i < r) out[i] = (uint8_t)(B[(N - (L - 1 + i)) & (N - 1)] & 1u);  // (L - 1 + i <= N - 1)
}

// Where a workgroup's LDS tile lies in the array: point l = (row << lc) | column is entry
// base + (row << rs) + column, rs = ls - c the log2 of the rows' distance.
struct TileMap {
    uint32_t base;
    int lc, rs;
    __device__ __forceinline__ uint32_t operator()(uint32_t l) const {
        return base + ((l >> lc) << rs) + (l & ((1u << lc) - 1u));
    }
};

enum { MODE_FWD = 0, MODE_INV = 1, MODE_MID = 2 };

// One stage on the tile: rows 2^hl apart, half size m = 2^(hl + rs) in the array.  LOCAL: the tile pass,
// whose table W[0 .. tile) is in LDS.  A thread takes its butterflies NTT_RUN at a time (all eight of a full
// tile): the run's loads are issued together, then its arithmetic and stores.  A butterfly past the tile's
// half (a short tile) loads the thread's first one again and stores nothing.
constexpr int NTT_RUN = NTT_TILE / 2 / NTT_THREADS;
template <bool DIT, bool LOCAL>
__device__ __forceinline__ void ntt_stage(uint32_t *pt, const uint32_t *tw, const uint32_t *W, const TileMap &g,
                                          int hl, int tl) {
    const int p = hl + g.lc;
    const uint32_t m = 1u << (hl + g.rs), half = (1u << tl) / 2;
    for (uint32_t b0 = threadIdx.x; b0 < half; b0 += NTT_THREADS * NTT_RUN) {
        uint32_t l0[NTT_RUN], w[NTT_RUN], x0[NTT_RUN], x1[NTT_RUN];
#pragma unroll
        for (int u = 0; u < NTT_RUN; ++u) {
            const uint32_t bu = b0 + u * NTT_THREADS, b = bu < half ? bu : b0;
            l0[u] = ((b >> p) << (p + 1)) | (b & ((1u << p) - 1u));
            const uint32_t idx = m + (g(l0[u]) & (m - 1u));
            w[u] = LOCAL ? tw[idx] : W[idx];
            x0[u] = pt[l0[u]];
            x1[u] = pt[l0[u] | (1u << p)];
        }
#pragma unroll
        for (int u = 0; u < NTT_RUN; ++u) {
            if (b0 + u * NTT_THREADS >= half) continue;
            const uint32_t l1 = l0[u] | (1u << p);
            if (DIT) {
                const uint32_t t = montmul(x1[u], w[u]);
                pt[l0[u]] = add_mod(x0[u], t);
                pt[l1] = sub_mod(x0[u], t);
            } else {
                pt[l0[u]] = add_mod(x0[u], x1[u]);
                pt[l1] = montmul(x0[u] - x1[u] + NTT_P, w[u]);
            }
        }
    }
    __syncthreads();
}

template <bool DIT, bool LOCAL>
__device__ __forceinline__ void ntt_stages(uint32_t *pt, const uint32_t *tw, const uint32_t *W, const TileMap &g,
                                           int c, int tl) {
    if (DIT)
        for (int hl = 0; hl < c; ++hl) ntt_stage<true, LOCAL>(pt, tw, W, g, hl, tl);
    else
        for (int hl = c - 1; hl >= 0; --hl) ntt_stage<false, LOCAL>(pt, tw, W, g, hl, tl);
}

// pt[l] = src[g(l)] over the tile (TIMES: pt[l] = pt[l] src[g(l)] scale / R^2), NTT_RUN loads in flight per thread
template <bool TIMES = false>
__device__ __forceinline__ void load_tile(uint32_t *pt, const uint32_t *src, const TileMap &g, uint32_t tile,
                                          uint32_t scale = 0) {
    for (uint32_t l0 = threadIdx.x; l0 < tile; l0 += NTT_THREADS * NTT_RUN) {
        uint32_t v[NTT_RUN];
#pragma unroll
        for (int u = 0; u < NTT_RUN; ++u) {
            const uint32_t l = l0 + u * NTT_THREADS;
            v[u] = src[g(l < tile ? l : l0)];  // (past a short tile: the thread's first point again, not stored)
        }
#pragma unroll
        for (int u = 0; u < NTT_RUN; ++u) {
            const uint32_t l = l0 + u * NTT_THREADS;
            if (l < tile) pt[l] = TIMES ? montmul(montmul(pt[l], v[u]), scale) : v[u];
        }
    }
}

// c stages of sub-transforms of 2^ls points on tiles of 2^c rows x 2^lc columns (c + lc <= NTT_TILE_LOG,
// ls - c >= lc).  LOCAL: the tile pass (ls == c, lc == 0), which alone keeps its table in LDS: a strided
// pass holds 16 KiB per workgroup, the tile pass 32.  MODE_MID (the tile pass only): forward, times spec
// and scale, backward.
template <int MODE, bool LOCAL>
__global__ void __launch_bounds__(NTT_THREADS) ntt_pass_kernel(uint32_t *x, const uint32_t *spec, const uint32_t *W,
                                                              int ls, int c, int lc, uint32_t scale) {
    static_assert(LOCAL || MODE != MODE_MID, "the middle pass is a tile pass");
    __shared__ uint32_t pt[NTT_TILE];
    __shared__ uint32_t tw[LOCAL ? NTT_TILE : 1];
    const int tl = c + lc, rs = ls - c, chunk_bits = rs - lc;
    const uint32_t tile = 1u << tl, wg = blockIdx.x;
    const TileMap g{((wg >> chunk_bits) << ls) + ((wg & ((1u << chunk_bits) - 1u)) << lc), lc, rs};
    load_tile(pt, x, g, tile);
    if (LOCAL)
        for (uint32_t l = threadIdx.x; l < tile; l += NTT_THREADS) tw[l] = W[l];
    __syncthreads();
    if (MODE == MODE_MID) {
        ntt_stages<false, LOCAL>(pt, tw, W, g, c, tl);
        load_tile<true>(pt, spec, g, tile, scale);
        __syncthreads();
        ntt_stages<true, LOCAL>(pt, tw, W, g, c, tl);
    } else {
        ntt_stages<MODE == MODE_INV, LOCAL>(pt, tw, W, g, c, tl);
    }
    for (uint32_t l = threadIdx.x; l < tile; l += NTT_THREADS) x[g(l)] = pt[l];
}

// ---- the host's share: the constants of a call ----
uint32_t host_to_mont(uint32_t v, uint32_t r2) { return montmul(v, r2); }
uint32_t host_pow(uint32_t base_m, uint64_t e, uint32_t one_m) {  // Montgomery forms in and out
    uint32_t v = one_m;
    for (; e; e >>= 1, base_m = montmul(base_m, base_m))
        if (e & 1) v = montmul(v, base_m);
    return v;
}

struct Pass {
    int ls, c, lc;
};

#define LAUNCH_TRY(...)                                     \
    do {                                                    \
        hipLaunchKernelGGL(__VA_ARGS__);                    \
        const hipError_t _e = hipGetLastError();            \
        if (_e != hipSuccess) return _e;                    \
    } while (0)

}  // namespace

hipError_t launch_toeplitz_block(int n_list, const int32_t *list, int key_len, long long key_stride,
                                 const uint8_t *keys, long long out_len, const uint8_t *seed, uint8_t *out, void *ws,
                                 hipStream_t stream) {
    const long long L = (long long)n_list * key_len, S = L + out_len - 1;
    const int k = toeplitz_block_log2(L, out_len);
    if (n_list <= 0 || k < 0) return hipErrorInvalidValue;
    const uint32_t N = 1u << k;
    uint32_t *A = reinterpret_cast<uint32_t *>((reinterpret_cast<uintptr_t>(ws) + 15) & ~(uintptr_t)15);
    uint32_t *B = A + N, *W = B + N;

    // Montgomery forms of 1, of w_N = 31^((P - 1) / N) and its squarings, and K = N^-1 R^2 mod P
    const uint32_t r1 = (uint32_t)((1ull << 32) % NTT_P), r2 = (uint32_t)((uint64_t)r1 * r1 % NTT_P);
    NttRoots roots;
    roots.one = r1;
    roots.pw[0] = host_pow(host_to_mont(NTT_ROOT, r2), (NTT_P - 1) >> k, r1);
    for (int b = 1; b < 27; ++b) roots.pw[b] = montmul(roots.pw[b - 1], roots.pw[b - 1]);
    const uint32_t scale = host_to_mont(host_pow(host_to_mont(N, r2), NTT_P - 2, r1), r2);  // (N^-1 R) R

    // the strided passes from the top, then the tile pass
    Pass up[(27 - NTT_TILE_LOG + NTT_PASS_STAGES - 1) / NTT_PASS_STAGES];
    const int tl = k < NTT_TILE_LOG ? k : NTT_TILE_LOG, ku = k - tl;
    const int n_up = (ku + NTT_PASS_STAGES - 1) / NTT_PASS_STAGES;
    for (int i = 0, ls = k; i < n_up; ++i) {
        const int c = ku / n_up + (i < ku % n_up ? 1 : 0);
        up[i] = Pass{ls, c, NTT_TILE_LOG - c};
        ls -= c;
    }
    const dim3 T(NTT_THREADS), tiles(N >> tl), points((N + NTT_THREADS - 1) / NTT_THREADS);

    const int lg = k - 1 < 16 ? (k - 1 < 0 ? 0 : k - 1) : 16;
    LAUNCH_TRY(block_twiddles_kernel, dim3(((1u << lg) + NTT_THREADS - 1) / NTT_THREADS), T, 0, stream, W, k, lg,
               roots);
    LAUNCH_TRY(block_pack_kernel, points, T, 0, stream, N, (uint32_t)L, (uint32_t)S, (uint32_t)key_len, key_stride,
               list, keys, seed, A, B);
    for (uint32_t *x : {A, B}) {
        for (int i = 0; i < n_up; ++i)
            LAUNCH_TRY((ntt_pass_kernel<MODE_FWD, false>), dim3(N >> NTT_TILE_LOG), T, 0, stream, x, nullptr, W,
                       up[i].ls, up[i].c, up[i].lc, 0u);
        if (x == A)
            LAUNCH_TRY((ntt_pass_kernel<MODE_FWD, true>), tiles, T, 0, stream, A, nullptr, W, tl, tl, 0, 0u);
        else
            LAUNCH_TRY((ntt_pass_kernel<MODE_MID, true>), tiles, T, 0, stream, B, A, W, tl, tl, 0, scale);
    }
    for (int i = n_up - 1; i >= 0; --i)
        LAUNCH_TRY((ntt_pass_kernel<MODE_INV, false>), dim3(N >> NTT_TILE_LOG), T, 0, stream, B, nullptr, W, up[i].ls,
                   up[i].c, up[i].lc, 0u);
    LAUNCH_TRY(block_extract_kernel, dim3((unsigned)((out_len + NTT_THREADS - 1) / NTT_THREADS)), T, 0, stream, N,
               (uint32_t)L, (uint32_t)out_len, B, out);
    return hipSuccess;
}

}  // namespace qldpc
