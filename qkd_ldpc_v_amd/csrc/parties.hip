// parties.hip — the per-party cut of the frame construction.
//
// The fused builders (decoder.hip build_frames_kernel, trials.hip
// build_frames_ra_kernel) restate the reference's simulation, which holds
// Alice's and Bob's keys side by side (src/qkd_ldpc_algorithm.cpp:1031-1119,
// :1121-1258).  In error reconciliation itself each side holds one key:
//   - Alice publishes the syndrome of her (extended) key: alice_syndrome_kernel;
//   - Bob turns his key and a QBER estimate into the decoder's input — f64 LLRs
//     or the V2 palette form, byte for byte what the fused builders write —
//     and decodes against the received syndrome: bob_frames_kernel;
//   - with a rate plan, Bob's decoded n-bit frame maps back to his n_key key
//     bits by the inverse of the extension: extract_key_kernel.
// One workgroup per frame; a party's key (and, for Alice with a plan, her
// punctured fill and the extended key) lives in LDS as bit words, so every
// gather (by src, by label, by row) reads LDS.  Key bytes are 0 or 1: only bit
// 0 is read.  Every global store is a plain vector store.
#include "decoder_common.hpp"

namespace qldpc {

namespace {

// cls == NULL: no plan, the extended key is the key.  With a plan the frame's
// key row is n bytes of which src[] names the first n - n_punct - n_short
// (QKD_LDPC_RATE_ADAPT reads alice_bit_array[n] the same way, :1169-1172);
// position i of the extended key is key[src[i]] (cls 0), fill[src[i]] (cls 1:
// Alice's private draws, :1148-1157) or 0 (cls 2).
__global__ void __launch_bounds__(1024) alice_syndrome_kernel(int n, int m, const int32_t *ell_col,
                                                             const int32_t *row_deg, const uint8_t *cls,
                                                             const int32_t *src, int n_punct, const uint8_t *key,
                                                             const uint8_t *fill, uint8_t *key_ext, uint8_t *synd) {
    extern __shared__ uint32_t kb[];
    const int nw = (n + 31) / 32, pw = (n_punct + 31) / 32, xw = 2 * ((n + 63) / 64);
    uint32_t *abits = kb, *pbits = kb + nw, *xbits = cls ? kb + nw + pw : kb;
    const size_t f = blockIdx.x;
    dev::pack_key_bits(key + f * (size_t)n, n, abits);
    if (cls && n_punct > 0) dev::pack_key_bits(fill + f * (size_t)n_punct, n_punct, pbits);
    __syncthreads();
    if (cls) {
        // the extended key, 64 positions per wave ballot
        const int lane = threadIdx.x & 63;
        for (int base = (int)(threadIdx.x & ~63u); base < 32 * xw; base += blockDim.x) {
            const int i = base + lane;
            uint32_t bit = 0;
            if (i < n) {
                const int c = cls[i];
                bit = c == 0 ? dev::key_bit(abits, src[i]) : (c == 1 ? dev::key_bit(pbits, src[i]) : 0u);
            }
            const uint64_t bal = __ballot(bit);
            if (lane == 0) {
                xbits[base >> 5] = (uint32_t)bal;
                xbits[(base >> 5) + 1] = (uint32_t)(bal >> 32);
            }
        }
        __syncthreads();
        if (key_ext) {
            uint8_t *ax = key_ext + f * (size_t)n;
            for (int i = threadIdx.x; i < n; i += blockDim.x) ax[i] = (uint8_t)dev::key_bit(xbits, i);
        }
    }
    uint8_t *s = synd + f * (size_t)m;
    for (int j = threadIdx.x; j < m; j += blockDim.x) s[j] = (uint8_t)dev::row_parity(xbits, ell_col, row_deg, m, j);
}

// Bob's side of the frame: palette code of position i is his key bit (0 / 1:
// +-log_p), 2 at a punctured position (ALMOST_ZERO = 1e-4 whatever he would
// draw there, :1153-1155) or 3 at a shortened one (DBL_MAX).  cls == NULL: no
// plan, codes 0 / 1 only and the palette's unused entries repeat entry 0.
__global__ void __launch_bounds__(1024) bob_frames_kernel(int n, const uint8_t *cls, const int32_t *src,
                                                         const uint8_t *key, const double *log_p, double *llr,
                                                         uint8_t *codes, double *palette, uint8_t *pal_ok,
                                                         const int32_t *col_orig) {
    extern __shared__ uint32_t kb[];
    uint32_t *bbits = kb;
    const size_t f = blockIdx.x;
    const double lp = log_p[f];
    dev::pack_key_bits(key + f * (size_t)n, n, bbits);
    __syncthreads();
    auto bob_code = [&](int i) -> int {
        if (!cls) return (int)dev::key_bit(bbits, i);
        const int c = cls[i];
        if (c == 0) return (int)dev::key_bit(bbits, src[i]);
        return c == 1 ? 2 : 3;
    };
    if (llr) {
        double *l = llr + f * (size_t)n;
        for (int i = threadIdx.x; i < n; i += blockDim.x) {
            const int code = bob_code(i);
            l[i] = code == 0 ? lp : code == 1 ? -lp : code == 2 ? 1e-4 : 1.7976931348623157e308;
        }
    }
    if (codes) {
        const int nc = (n + 3) / 4;
        uint8_t *cs = codes + f * (size_t)nc;
        for (int j = threadIdx.x; j < nc; j += blockDim.x) {
            int byte = 0;
            for (int q = 0; q < 4; ++q) {  // label order (col_orig)
                const int i = 4 * j + q;
                if (i < n) byte |= bob_code(col_orig ? col_orig[i] : i) << (2 * q);
            }
            cs[j] = (uint8_t)byte;
        }
        if (threadIdx.x < 4) {
            const double pv[4] = {lp, -lp, cls ? 1e-4 : lp, cls ? 1.7976931348623157e308 : lp};
            palette[f * 4 + threadIdx.x] = pv[threadIdx.x];
        }
        if (threadIdx.x == 0) pal_ok[f] = 1;
    }
}

// out[f][src[i]] = bits[f][i] for every key position i (cls 0): src ascends
// over them, so a wave's reads are contiguous and its writes nearly so.
__global__ void __launch_bounds__(1024) extract_key_kernel(int n, int n_key, const uint8_t *cls,
                                                          const int32_t *src, const uint8_t *bits, uint8_t *out) {
    const size_t f = blockIdx.x;
    const uint8_t *b = bits + f * (size_t)n;
    uint8_t *o = out + f * (size_t)n_key;
    for (int i = threadIdx.x; i < n; i += blockDim.x)
        if (cls[i] == 0) o[src[i]] = b[i];
}

template <typename K>
hipError_t dynamic_lds(K kernel, size_t lds) {
    if (lds > LDS_MAX_BYTES) return hipErrorInvalidValue;
    if (lds > 65536) return allow_dynamic_lds(reinterpret_cast<const void *>(kernel), lds);
    return hipSuccess;
}

}  // namespace

hipError_t launch_alice_syndrome(int n, int m, const int32_t *ell_col, const int32_t *row_deg, const uint8_t *cls,
                                 const int32_t *src, int n_punct, int batch, const uint8_t *key,
                                 const uint8_t *fill, uint8_t *key_ext, uint8_t *synd, hipStream_t stream) {
    if (batch <= 0) return hipSuccess;
    const size_t lds = alice_syndrome_lds(n, cls ? n_punct : -1);
    const hipError_t e = dynamic_lds(alice_syndrome_kernel, lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(alice_syndrome_kernel, dim3(batch), dim3(aux_frame_threads(n)), lds, stream, n, m, ell_col,
                       row_deg, cls, src, cls ? n_punct : 0, key, fill, key_ext, synd);
    return hipGetLastError();
}

hipError_t launch_bob_frames(int n, const uint8_t *cls, const int32_t *src, int batch, const uint8_t *key,
                             const double *log_p, double *llr, uint8_t *codes, double *palette, uint8_t *pal_ok,
                             const int32_t *col_orig, hipStream_t stream) {
    if (batch <= 0) return hipSuccess;
    const size_t lds = bob_frames_lds(n);
    const hipError_t e = dynamic_lds(bob_frames_kernel, lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(bob_frames_kernel, dim3(batch), dim3(aux_frame_threads(n)), lds, stream, n, cls, src, key, log_p,
                       llr, codes, palette, pal_ok, col_orig);
    return hipGetLastError();
}

hipError_t launch_extract_key(int n, int n_key, const uint8_t *cls, const int32_t *src, int batch,
                              const uint8_t *bits, uint8_t *out, hipStream_t stream) {
    if (batch <= 0 || n_key <= 0) return hipSuccess;
    hipLaunchKernelGGL(extract_key_kernel, dim3(batch), dim3(aux_frame_threads(n)), 0, stream, n, n_key, cls, src, bits,
                       out);
    return hipGetLastError();
}

}  // namespace qldpc
