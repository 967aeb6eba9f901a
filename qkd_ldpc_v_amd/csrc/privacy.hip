// privacy.hip — a batched Toeplitz hash over GF(2): key verification (a short
// tag) and privacy amplification (a long output, per-frame lengths) of the
// keys that reconciliation leaves on the device.
//
// For a frame's key x[0..L), the batch's public seed s[0..L+r-1) and r outputs:
//     y[i] = XOR over j in [0, L) of  s[i + L - 1 - j] & x[j]
// (the Toeplitz matrix T[i][j] = s[i - j + L - 1]).  Row i reads s[i .. i+L)
// only, so the first r' outputs are the hash for out_len = r'.
//
// A workgroup takes HASH_TILE consecutive outputs [o0, o0 + TO) of HASH_FRAMES
// consecutive frames.  TO is the tile cut to the longest of its frames'
// lengths.  The seed is packed into LDS REVERSED from the tile's end,
//     R[v] = s[o0 + TO + L - 2 - v],
// so that output o0 + t is the sliding correlation of the forward key (packed by
// dev::pack_key_bits, as everywhere) at offset q = TO - 1 - t:
//     y[o0 + t] = parity of  AND over words w of  R[q + 32 w .. q + 32 w + 32) & X[w].
// A wave owns 256 consecutive offsets, a lane the HASH_SLOTS offsets
// q = 32 (B + kk) + (lane & 31), kk < HASH_SLOTS, from its word base
// B = 8 wave + 4 (lane >> 5): its shift q & 31 is one value and its slots are
// one seed word apart.  For four key words w .. w + 3 the lane's slots read
// the eight seed words R[B + w .. B + w + 8) — two 16-byte LDS loads, the first
// of them the previous step's second — and slot kk at key word w + j wants the
// window that starts at seed word B + w + kk + j: seven funnel shifts of
// neighbouring words serve the sixteen (slot, word) pairs.  The seed words are
// one address per wave half, a key word one per wave (both broadcast), and a
// window is shared by the workgroup's frames in registers; each pair costs one
// fused AND-XOR per frame, parity taken once at the end.  Every global store is
// a plain vector store.
#include "decoder_common.hpp"

namespace qldpc {

namespace {

constexpr int HASH_SLOTS = HASH_TILE / HASH_THREADS;  // offsets per lane

__device__ __forceinline__ uint32_t word_of(const uint4 &v, int j) {
    return j == 0 ? v.x : j == 1 ? v.y : j == 2 ? v.z : v.w;
}

// The first NK slots of the wave's lanes (the others lie past the tile's end).
// kw4: the key's words rounded up to a multiple of 4 (the pad words are zero,
// so is every key bit past L: the seed bits they meet do not count).
template <int NK>
__device__ __forceinline__ void hash_slots(const uint32_t *kbits, int kw4, const uint32_t *rbits, int wave, int lane,
                                           uint32_t (&acc)[HASH_SLOTS][HASH_FRAMES]) {
    const uint32_t sh = (uint32_t)lane & 31u;
    const uint4 *r4 = reinterpret_cast<const uint4 *>(rbits) + 2 * wave + (lane >> 5);  // word base B = 8 wave + 4 half
    uint4 cur = r4[0];
    for (int w = 0; w < kw4; w += 4) {
        const uint4 nxt = r4[w / 4 + 1];
        uint4 x[HASH_FRAMES];
#pragma unroll
        for (int f = 0; f < HASH_FRAMES; ++f) x[f] = *reinterpret_cast<const uint4 *>(kbits + (size_t)f * kw4 + w);
        uint32_t win[NK + 3];  // win[i]: the 32 seed bits from bit sh of word B + w + i (sh == 0: the word itself)
#pragma unroll
        for (int i = 0; i < NK + 3; ++i)
            win[i] = __funnelshift_r(i < 4 ? word_of(cur, i) : word_of(nxt, i - 4),
                                     i < 3 ? word_of(cur, i + 1) : word_of(nxt, i - 3), sh);
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int kk = 0; kk < NK; ++kk)
#pragma unroll
                for (int f = 0; f < HASH_FRAMES; ++f)  // acc ^ (win & key word): one VALU operation
                    acc[kk][f] = __builtin_amdgcn_bitop3_b32(win[kk + j], acc[kk][f], word_of(x[f], j), 0x6c);
        cur = nxt;
    }
}

__global__ void __launch_bounds__(HASH_THREADS) toeplitz_hash_kernel(int batch, int L, long long key_stride,
                                                                    const uint8_t *keys, int r, const uint8_t *seed,
                                                                    const int32_t *out_len, uint8_t *out) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const int kw = (L + 31) / 32, kw4 = (kw + 3) & ~3, rw = hash_seed_words(L);
    uint32_t *kbits = lds, *rbits = lds + (size_t)HASH_FRAMES * kw4;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t f0 = (size_t)blockIdx.x * HASH_FRAMES;
    const long long o0 = (long long)blockIdx.y * HASH_TILE;
    const int tile = (int)(r - o0 < HASH_TILE ? r - o0 : HASH_TILE);  // this tile's columns of the output

    // the frames' lengths (clamped into [0, r]) relative to the tile, and the longest of them
    int len[HASH_FRAMES], TO = 0;
#pragma unroll
    for (int f = 0; f < HASH_FRAMES; ++f) {
        long long l = 0;
        if (f0 + f < (size_t)batch) {
            l = out_len ? (long long)out_len[f0 + f] : (long long)r;
            l = (l < 0 ? 0 : l > r ? r : l) - o0;
        }
        len[f] = (int)(l < 0 ? 0 : l > tile ? tile : l);
        TO = len[f] > TO ? len[f] : TO;
    }
    // columns no frame of the workgroup reaches: zeros
#pragma unroll
    for (int f = 0; f < HASH_FRAMES; ++f) {
        if (f0 + f >= (size_t)batch) continue;
        uint8_t *o = out + (f0 + f) * (size_t)r + o0;
        for (int t = TO + threadIdx.x; t < tile; t += HASH_THREADS) o[t] = 0;
    }
    if (TO == 0) return;  // (the whole workgroup: nothing to hash)

    // the keys, forward, HASH_FRAMES rows of kw4 words; a frame past the batch is all zero
#pragma unroll
    for (int f = 0; f < HASH_FRAMES; ++f) {
        uint32_t *kb = kbits + (size_t)f * kw4;
        const bool live = f0 + f < (size_t)batch;
        if (live) dev::pack_key_bits(keys + (f0 + f) * (size_t)key_stride, L, kb);
        for (int w = (live ? kw : 0) + threadIdx.x; w < kw4; w += HASH_THREADS) kb[w] = 0;
    }
    // the seed, reversed from the tile's end: R[v] = s[o0 + TO + L - 2 - v] for v <= TO + L - 2, else 0;
    // 64 positions per wave ballot (rw is even), SEED_RUN loads in flight per lane before the first ballot
    const long long top = o0 + TO + L - 2;  // <= r + L - 2, the seed's last entry
    const int vmax = TO + L - 2;
    constexpr int SEED_RUN = 8;
    for (int base = 64 * SEED_RUN * wave; base < 32 * rw; base += HASH_THREADS * SEED_RUN) {
        uint32_t bit[SEED_RUN];
#pragma unroll
        for (int u = 0; u < SEED_RUN; ++u) {
            const int v = base + 64 * u + lane;
            bit[u] = v <= vmax ? (seed[top - v] & 1u) : 0u;  // (v past the window's words: 0, and not stored)
        }
#pragma unroll
        for (int u = 0; u < SEED_RUN; ++u) {
            const uint64_t bal = __ballot(bit[u]);
            const int w = (base >> 5) + 2 * u;
            if (lane == 0 && w < rw) {
                rbits[w] = (uint32_t)bal;
                rbits[w + 1] = (uint32_t)(bal >> 32);
            }
        }
    }
    __syncthreads();

    // the wave's offsets start at 256 wave; its slots kk start at 256 wave + 32 kk: a wave past the tile's
    // end hashes nothing
    const int first = 256 * wave, want = first >= TO ? 0 : (TO - first + 31) / 32;
    const int nk = want < HASH_SLOTS ? want : HASH_SLOTS;
    uint32_t acc[HASH_SLOTS][HASH_FRAMES] = {};
    static_assert(HASH_SLOTS == 4 && HASH_THREADS == 256, "one case per slot count; 256 offsets per wave");
    switch (nk) {
        case 0: return;
        case 1: hash_slots<1>(kbits, kw4, rbits, wave, lane, acc); break;
        case 2: hash_slots<2>(kbits, kw4, rbits, wave, lane, acc); break;
        case 3: hash_slots<3>(kbits, kw4, rbits, wave, lane, acc); break;
        default: hash_slots<4>(kbits, kw4, rbits, wave, lane, acc); break;
    }
#pragma unroll
    for (int kk = 0; kk < HASH_SLOTS; ++kk) {
        const int t = TO - 1 - (first + 128 * (lane >> 5) + 32 * kk + (lane & 31));
        if (kk >= nk || t < 0) continue;
#pragma unroll
        for (int f = 0; f < HASH_FRAMES; ++f) {
            if (f0 + f >= (size_t)batch) continue;
            out[(f0 + f) * (size_t)r + o0 + t] = t < len[f] ? (uint8_t)(__popc(acc[kk][f]) & 1) : (uint8_t)0;
        }
    }
}

}  // namespace

hipError_t launch_toeplitz_hash(int batch, int key_len, long long key_stride, const uint8_t *keys, int out_len,
                                const uint8_t *seed, const int32_t *out_lens, uint8_t *out, hipStream_t stream) {
    if (batch <= 0) return hipSuccess;
    const size_t lds = toeplitz_hash_lds(key_len);
    if (lds > LDS_MAX_BYTES || !toeplitz_hash_grid_ok(batch, out_len)) return hipErrorInvalidValue;
    if (lds > 65536) {
        const hipError_t e = allow_dynamic_lds(reinterpret_cast<const void *>(toeplitz_hash_kernel), lds);
        if (e != hipSuccess) return e;
    }
    const dim3 grid((unsigned)((batch + HASH_FRAMES - 1) / HASH_FRAMES),
                    (unsigned)(((long long)out_len + HASH_TILE - 1) / HASH_TILE));
    hipLaunchKernelGGL(toeplitz_hash_kernel, grid, dim3(HASH_THREADS), lds, stream, batch, key_len, key_stride, keys,
                       out_len, seed, out_lens, out);
    return hipGetLastError();
}

}  // namespace qldpc
