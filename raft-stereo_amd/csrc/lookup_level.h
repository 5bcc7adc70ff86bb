// Per-level window lookup shared by lookup.hip and lookup_conv_bwd.hip: the
// pixel's x coordinate, one level's window loads (issue_level) and its taps
// (finish_level).  The arithmetic is documented at the top of lookup.hip;
// every user must be built with -ffp-contract=off.
#pragma once
#include "common.h"

namespace rc {

// x coordinate of pixel (bimg, rem).  For rc_corr_lookup_step the pixel's
// coordinates are first advanced by the previous iteration's update (the
// forward loop's tail, SURVEY Appendix A D8: coords1 + delta_flow with the
// y component zeroed) and the new coords and flow = coords1 - coords0
// (model.py:377, coords0 = coords_grid, :329-332) are written -- the
// loop's per-iteration elementwise ops, fused into the lookup launch.
__device__ __forceinline__ float pixel_x(const LookupArgs &a, long long bimg, long long rem,
                                         bool active) {
    if (!a.step) return a.coords[bimg * a.cbs + rem];
    const long long o = bimg * 2LL * a.HW + rem;   // (B,2,H,W1) contiguous
    float x = a.coords[o];
    float y = a.coords[o + a.HW];
    if (a.delta) {
        x = x + a.delta[o];
        y = y + 0.0f;                               // delta_flow[:,1] = 0
    }
    if (active) {
        const int h = (int)(rem / a.W1), w = (int)(rem - (long long)h * a.W1);
        a.coords_out[o] = x;
        a.coords_out[o + a.HW] = y;
        a.flow_out[o] = x - (float)w;
        a.flow_out[o + a.HW] = y - (float)h;
    }
    return x;
}

// EK: the pyramid's element kind (kF32 / kBF16 / kF16; a kernel's `bool BF16`
// converts to the first two).
template <int R, int EK>
struct LevelWindow {
    static constexpr int T = 2 * R + 1;
    static constexpr int NW = 2 * R + 4;              // window elements
    static constexpr int EPV = EK != kF32 ? 8 : 4;    // elements per 16-B load
    static constexpr int NV = (NW + 2 * (EPV - 1)) / EPV;
    static constexpr int ES = EK != kF32 ? 2 : 4;
    uint32_t q[NV][4];                                 // raw loaded dwords
    float xp[T];
    float n;
    int sh;
    bool inwin;
};

template <int R, int EK, bool EXACT>
__device__ __forceinline__ void issue_level(LevelWindow<R, EK> &lw, const LookupArgs &a, int i,
                                            float x, long long pblk, long long lrow) {
    typedef LevelWindow<R, EK> LW;
    const int W = a.W[i];
    const long long ld = a.ld[i];
    const float Wm1 = (float)(W - 1);
    const DivRN dv = div_prep(Wm1);
    const float half = Wm1 / 2.0f;
    const float xl = x / (float)(1 << i);
#pragma unroll
    for (int t = 0; t < LW::T; ++t) {
        const float xt = (float)(t - R) + xl;
        const float xn = div_rn(2.0f * xt, dv) - 1.0f;
        lw.xp[t] = (xn + 1.0f) * half;
    }
    lw.inwin = (xl > -(float)(R + 4)) && (xl < (float)(W + R + 4));  // false for NaN
    lw.n = lw.inwin ? floorf(xl) : 0.0f;
    const long long e = lrow * ld + (long long)lw.n - (R + 1);
    const long long ea = e & ~(long long)(LW::EPV - 1);
    lw.sh = (int)(e - ea);
    // exact span of elements the taps read, clipped to the row's [0, W): the
    // zero padding masks everything outside (relative to the block base;
    // selects on floats first: a NaN/huge float must never reach an integer cast)
    const float f0 = lw.inwin ? fmaxf(floorf(lw.xp[0]), 0.0f) : 0.0f;
    const float f1 = lw.inwin ? fminf(floorf(lw.xp[LW::T - 1]) + 1.0f, Wm1) : -1.0f;
    const bool any = lw.inwin && f0 <= f1;
    const long long first = lrow * ld + (long long)f0;
    const long long last = lrow * ld + (long long)f1;
    const char *base = reinterpret_cast<const char *>(a.lvl[i]) + pblk * ld * LW::ES;
    const auto rs = make_rsrc(base, clamp_bytes((a.P - pblk) * ld * LW::ES));
#pragma unroll
    for (int k = 0; k < LW::NV; ++k) {
        const long long c0 = ea + (long long)k * LW::EPV;
        uint32_t off = (uint32_t)(c0 * LW::ES);
        if (EXACT && !(any && c0 <= last && c0 + LW::EPV - 1 >= first)) off = 0xFFFFFF00u;
        const auto v = __builtin_amdgcn_raw_buffer_load_b128(rs, (int)off, 0, 0);
#pragma unroll
        for (int c = 0; c < 4; ++c) lw.q[k][c] = v[c];
    }
}

template <int R, int EK, class Sink>
__device__ __forceinline__ void finish_level(const LevelWindow<R, EK> &lw, const LookupArgs &a,
                                             int i, long long pblk, long long lrow, Sink &&sink) {
    typedef LevelWindow<R, EK> LW;
    constexpr int T = LW::T, NW = LW::NW, EPV = LW::EPV, NE = LW::NV * EPV;
    const int W = a.W[i];
    const float Wm1 = (float)(W - 1);
    float v[NE];
#pragma unroll
    for (int k = 0; k < LW::NV; ++k)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const uint32_t u = lw.q[k][c];
            if constexpr (EK != kF32) {
                v[k * 8 + 2 * c] = h16_lo(u, EK);
                v[k * 8 + 2 * c + 1] = h16_hi(u, EK);
            } else {
                v[k * 4 + c] = __builtin_bit_cast(float, u);
            }
        }
    // s[j] = element (n - R - 1 + j) = v[j + sh]
    float s[NW];
#pragma unroll
    for (int j = 0; j < NW; ++j) {
        float r = v[j];
#pragma unroll
        for (int k = 1; k < EPV; ++k) r = (lw.sh == k) ? v[j + k] : r;
        s[j] = r;
    }
    // fast path for every tap, then ONE wave-level check for the (unreachable
    // within the error bound) taps whose floor left the window
    float res[T];
    bool bad = false;
#pragma unroll
    for (int t = 0; t < T; ++t) {
        const float xp = lw.xp[t];
        const float x0 = floorf(xp);
        const float w1 = xp - x0, w0 = 1.0f - w1;
        const float nt = lw.n + (float)(t - R);
        const bool lo = x0 < nt, hi = x0 > nt;
        const float a0 = lo ? s[t] : (hi ? s[t + 2] : s[t + 1]);
        const float a1 = lo ? s[t + 1] : (hi ? s[t + 3] : s[t + 2]);
        const bool ok0 = (x0 >= 0.0f) && (x0 <= Wm1);
        const bool ok1 = (x0 + 1.0f >= 0.0f) && (x0 + 1.0f <= Wm1);
        bad |= lw.inwin && (x0 < nt - 1.0f || x0 > nt + 1.0f);
        const float v0 = ok0 ? a0 : 0.0f;
        const float v1 = ok1 ? a1 : 0.0f;
        res[t] = fmaf(w1, v1, w0 * v0);
    }
    if (__builtin_expect(bad, 0)) {
        // Guarded scalar fallback: re-read every tap of this lane from memory.
        const char *base = reinterpret_cast<const char *>(a.lvl[i]) + pblk * a.ld[i] * LW::ES;
        for (int t = 0; t < T; ++t) {
            const float xp = lw.xp[t];
            const float x0 = floorf(xp);
            const float w1 = xp - x0, w0 = 1.0f - w1;
            const bool ok0 = (x0 >= 0.0f) && (x0 <= Wm1);
            const bool ok1 = (x0 + 1.0f >= 0.0f) && (x0 + 1.0f <= Wm1);
            const long long k0 = lrow * a.ld[i] + (long long)x0;
            float v0 = 0.0f, v1 = 0.0f;
            if constexpr (EK != kF32) {
                const uint16_t *rowp = reinterpret_cast<const uint16_t *>(base);
                if (ok0) v0 = h16_to_f32(rowp[k0], EK);
                if (ok1) v1 = h16_to_f32(rowp[k0 + 1], EK);
            } else {
                const float *rowp = reinterpret_cast<const float *>(base);
                if (ok0) v0 = rowp[k0];
                if (ok1) v1 = rowp[k0 + 1];
            }
            res[t] = fmaf(w1, v1, w0 * v0);
        }
    }
#pragma unroll
    for (int t = 0; t < T; ++t) sink(t, res[t]);
}

}  // namespace rc
