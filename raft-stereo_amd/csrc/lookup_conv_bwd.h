// The part of the fused lookup+convc1 backward that does not depend on how
// the lane obtained its pixel's corr[]: shared by lookup_conv_bwd_kernel
// (per-level recompute, lookup_conv_bwd.hip) and lookup_pair_conv_grad_kernel
// (pair-span recompute, lookup_pair_conv.hip).  See lookup_conv_bwd.hip for
// the scheme; with the same corr bits, the same pixel-to-workgroup assignment
// (workgroup b owns pixels [256 b, 256 b + 256), lane = pixel) and the same
// summation order, both kernels give the same gradients bit for bit.
#pragma once
#include "common.h"

namespace rc {

constexpr int kCbwdPitch = 68;                 // LDS row pitch (floats)
constexpr int kCbwdGTile = 16 * kCbwdPitch;    // one wave's g[16][64] tile

// column tiles of the sums: corr channels + the ones column
template <int CIN>
constexpr int cbwd_tiles() { return (CIN + 1 + 15) / 16; }

// s_corr: 4 * CIN * kCbwdPitch floats, s_g: 4 * kCbwdGTile floats (LDS of the
// calling kernel).  bimg, rem: the lane's pixel (pixel P-1 for inactive lanes).
template <int CIN>
__device__ __forceinline__ void conv_bwd_sums(const float (&corr)[CIN], const LookupArgs &a, bool active,
                                              long long bimg, long long rem, float *s_corr, float *s_g,
                                              const float *__restrict__ wgt, const float *__restrict__ bias,
                                              int cout, int relu, const float *__restrict__ gout,
                                              float *__restrict__ gcorr, float *__restrict__ ws) {
    constexpr int NT = cbwd_tiles<CIN>();
    static_assert(NT * 4 * 64 <= kCbwdGTile, "fragment exchange reuses the g tile");
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    float *sc = s_corr + wave * CIN * kCbwdPitch, *sg = s_g + wave * kCbwdGTile;
    if (ws) {
        // lanes past the last pixel stand in for pixel P-1: zero, so that a
        // non-finite corr there cannot reach the sums (their g is zero too)
#pragma unroll
        for (int k = 0; k < CIN; ++k) sc[k * kCbwdPitch + lane] = active ? corr[k] : 0.0f;
    }
    float gc[CIN];
#pragma unroll
    for (int k = 0; k < CIN; ++k) gc[k] = 0.0f;
    const float *gop = gout + bimg * (long long)cout * a.HW + rem;
    const int i16 = lane & 15, g4 = lane >> 4;
    const long long wsn = (long long)cout * (CIN + 1);       // floats per workgroup slice
    for (int c0 = 0; c0 < cout; c0 += 16) {
#pragma unroll 1
        for (int cc = 0; cc < 16; ++cc) {
            const int c = c0 + cc;
            float g = 0.0f;
            if (c < cout) {                                   // block-uniform
                const float *wr = wgt + c * CIN;
                float acc = bias ? bias[c] : 0.0f;
#pragma unroll
                for (int k = 0; k < CIN; ++k) acc = fmaf(wr[k], corr[k], acc);
                const float go = active ? gop[(long long)c * a.HW] : 0.0f;
                g = (relu && !(acc > 0.0f)) ? 0.0f : go;
                if (gcorr) {
#pragma unroll
                    for (int k = 0; k < CIN; ++k) gc[k] = fmaf(wr[k], g, gc[k]);
                }
            }
            if (ws) sg[cc * kCbwdPitch + lane] = g;
        }
        if (!ws) continue;                                    // block-uniform
        __syncthreads();
        f32x4 acc[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[nt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            const int px = 4 * s + g4;                        // lane (i16, g4) supplies k = g4 of step s
            const float av = sg[i16 * kCbwdPitch + px];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const int j = 16 * nt + i16;
                const float cv = sc[(j < CIN ? j : CIN - 1) * kCbwdPitch + px];
                const float bv = j < CIN ? cv : (j == CIN ? 1.0f : 0.0f);
                acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc[nt], 0, 0, 0);
            }
        }
        // the wave's fragments over its own (already read) g tile, then the
        // four waves added in wave order: lane l, register r of tile nt is
        // row 4 (l >> 4) + r, column 16 nt + (l & 15)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int r = 0; r < 4; ++r) sg[(nt * 4 + r) * 64 + lane] = acc[nt][r];
        __syncthreads();
        for (int e = tid; e < NT * 256; e += 256) {
            const int q = e >> 6, l = e & 63;
            const int c = c0 + 4 * (l >> 4) + (q & 3), j = 16 * (q >> 2) + (l & 15);
            const float sum = ((s_g[e] + s_g[kCbwdGTile + e]) + s_g[2 * kCbwdGTile + e]) + s_g[3 * kCbwdGTile + e];
            if (c < cout && j <= CIN) ws[(long long)blockIdx.x * wsn + (long long)c * (CIN + 1) + j] = sum;
        }
        __syncthreads();                                      // the tiles are rewritten next round
    }
    if (gcorr && active) {
        float *gp = gcorr + bimg * (long long)CIN * a.HW + rem;
#pragma unroll
        for (int k = 0; k < CIN; ++k) gp[(long long)k * a.HW] = gc[k];
    }
}

}  // namespace rc

// the second launch of both backward kernels (lookup_conv_bwd.hip): adds the
// nblk workgroup slices of ws in a fixed order into grad_weight / grad_bias
hipError_t rc_launch_lookup_conv_bwd_reduce(const float *ws, int nblk, int cout, int cin, float *grad_weight,
                                            float *grad_bias, hipStream_t s);
