// The pair-layout lookup kernels (gfx950): lookup_pair_kernel, the disparity-
// major lookup_sheared_pair_kernel and lookup_records_kernel, with the span
// helpers they share.  Templates only: lookup.hip instantiates the fp32-output
// kernels, lookup_half.hip the fp16 / bf16-output ones (RC_OUT_F16 /
// RC_OUT_BF16), lookup_f16pyr.hip the ones that read an fp16 pyramid
// (RC_F16), so no translation unit pays for another's compile.
#pragma once
#include <type_traits>

#include "common.h"
#include "lookup_level.h"   // pixel_x

namespace rc {

// Output element of the pair / records kernels: float, or _Float16 / __bf16
// (RC_OUT_F16 / RC_OUT_BF16).  The final fp32 value is rounded to nearest
// even by the hardware convert (v_cvt_f16_f32, v_cvt_pk_bf16_f32): +-inf
// stays, fp16 overflow gives +-inf, fp16 subnormals are kept (the kernel's
// fp16 denormal mode is IEEE), NaN stays NaN -- what Tensor.to(dtype) does.
// The opaque copy keeps the rounded fp32 value a value: without it the
// compiler folds a tap's fmaf and this convert into one v_fma_mixlo_f16,
// which rounds the exact fma once, to fp16 -- not the fp32 output's rounding
// (seen as 2 of 16200 elements off by one fp16 ulp on the records kernel).
template <class OT>
__device__ __forceinline__ OT out_cvt(float v) {
    if constexpr (std::is_same<OT, float>::value) {
        return v;
    } else {
        asm("" : "+v"(v));
        return (OT)v;
    }
}

// pairwise-mean tree of S consecutive elements, the fp32 ops of model.py:294
template <int S>
__device__ __forceinline__ float pool_tree(const float *v) {
    if constexpr (S == 1) return v[0];
    else return (pool_tree<S / 2>(v) + pool_tree<S / 2>(v + S / 2)) * 0.5f;
}

// level-i element k (S_i = 2^(i-1) level-1 elements) straight from memory
template <int SI>
__device__ __forceinline__ float derived_elem(const float *row1, long long k) {
    float v[SI];
#pragma unroll
    for (int c = 0; c < SI; ++c) v[c] = row1[SI * k + c];
    return pool_tree<SI>(v);
}

// ---- lookup over a pool-chain pyramid stored as levels 0 and 2 ("pair") ----
// Level 2k+1 element j is the pairwise mean of level-2k elements 2j, 2j+1
// (model.py:294, the fp32 ops (a + b) * 0.5), so ONE span of level 2k feeds
// the windows of both levels 2k and 2k+1:
//   span  = level-2k elements [2(m-R-1), 2(m+R+3)),  m = floor(x / 2^(2k+1))
//   level 2k+1, window element jj (element m-R-1+jj) = mean(span[2jj], span[2jj+1])
//   level 2k,   window element jj (element n-R-1+jj) = span[dd+R+1+jj],
//               n = floor(x / 2^(2k)) = 2m + dd, dd in {0, 1}
// With 4 levels the build stores levels 0 and 2 only and a pixel reads two
// such spans (2(2r+4) elements each): ~2.8 128-B lines per pixel at the bench
// coordinates against ~3.0 for the level-1 chain (level-0 window + level-1
// span) and ~4.4 for one window per level, in 14 instead of
// 16 16-B loads per lane, and with fewer selects.  Window elements outside
// [0, W_level) are zeroed once per level, which is exactly the reference's
// per-tap zero padding (a tap reads window elements x0 and x0+1 only).
// EK: the pyramid's element kind (kF32 / kBF16 / kF16; a kernel's `bool BF16`
// converts to the first two) -- here and in every helper below.
template <int R, int EK = kF32>
struct PairSpan {
    static constexpr int NW = 2 * R + 4;              // window elements per level
    static constexpr int NS = 2 * NW;                 // span elements
    static constexpr int EPC = EK != kF32 ? 8 : 4;    // elements per 16-B chunk
    static constexpr int ES = EK != kF32 ? 2 : 4;     // element bytes
    // the span starts at an even element: misaligned by 0, 2, .., EPC-2
    static constexpr int NC = (NS + EPC - 2 + EPC - 1) / EPC;
    uint32_t q[NC][4];                                // raw chunks
    float m, n;                                       // window centres of the odd / even level
    float xe[4];                                      // x' of taps -R, +R of the even, then the odd level
    int sh;                                           // span start - chunk base (elements)
    bool inwin, valid;
    // element e of the loaded chunks, as fp32
    __device__ __forceinline__ float elem(int e) const {
        if constexpr (EK != kF32) {
            const uint32_t u = q[e >> 3][(e & 7) >> 1];
            return (e & 1) ? h16_hi(u, EK) : h16_lo(u, EK);
        } else {
            return __builtin_bit_cast(float, q[e >> 2][e & 3]);
        }
    }
};

// The sampler's per-level constants: Wm1 = W - 1, half = Wm1 / 2 and the
// Markstein divisor {Wm1, RN(1 / Wm1)}.
struct LevelConsts {
    float Wm1, half;
    DivRN dv;
};
__device__ __forceinline__ LevelConsts level_consts(const LookupArgs &a, int i) {
    const float Wm1 = (float)(a.W[i] - 1);
    return LevelConsts{Wm1, Wm1 / 2.0f, div_prep(Wm1)};
}

// x' of tap k of a level at x_l: the reference's normalise / unnormalise
// round trip (lookup.hip), fp32 op for op.
__device__ __forceinline__ float tap_xp(float xl, int k, const LevelConsts &c) {
    const float xt = (float)k + xl;
    const float xn = div_rn(2.0f * xt, c.dv) - 1.0f;
    return (xn + 1.0f) * c.half;
}

// The geometry of one pair's span for x: the window centres, and the exact
// element range [lo_e, hi_e] of level lo that the taps of both levels read
// (clipped to the rows; empty as lo_e > hi_e).  The x' of each level's two
// edge taps, which bound that range, are kept in ps.xe: window_taps takes
// them from there instead of evaluating them again.
template <int R, int EK>
__device__ __forceinline__ void plan_pair(PairSpan<R, EK> &ps, const LookupArgs &a, int lo, float x,
                                          int &lo_e, int &hi_e) {
    const int Wlo = a.W[lo], Whi = a.W[lo + 1];
    const float xlo = x / (float)(1 << lo), xhi = x / (float)(2 << lo);
    // false for NaN; outside it every tap of both levels is zero padding
    ps.inwin = (xhi > -(float)(R + 4)) && (xhi < (float)(Whi + R + 4));
    ps.m = ps.inwin ? floorf(xhi) : 0.0f;
    ps.n = ps.inwin ? floorf(xlo) : 0.0f;
    const int dd = (int)ps.n - 2 * (int)ps.m;
    ps.valid = ps.inwin && (dd == 0 || dd == 1);      // a subnormal x can break it
    const LevelConsts clo = level_consts(a, lo), chi = level_consts(a, lo + 1);
    ps.xe[0] = tap_xp(xlo, -R, clo);
    ps.xe[1] = tap_xp(xlo, R, clo);
    ps.xe[2] = tap_xp(xhi, -R, chi);
    ps.xe[3] = tap_xp(xhi, R, chi);
    lo_e = 0x7FFFFFFF;
    hi_e = -1;
    if (ps.inwin) {    // integer casts of in-window (finite, bounded) values only
        int f = max((int)floorf(ps.xe[0]), 0), l = min((int)floorf(ps.xe[1]) + 1, Wlo - 1);
        if (f <= l) { lo_e = f; hi_e = l; }
        f = max((int)floorf(ps.xe[2]), 0);
        l = min((int)floorf(ps.xe[3]) + 1, Whi - 1);
        if (f <= l) { lo_e = min(lo_e, 2 * f); hi_e = max(hi_e, 2 * l + 1); }
    }
}

// The loads of one pair's span: the buffer resource and the byte offset of
// each 16-B chunk (an out-of-range offset where the taps read none of it).
template <int R, int EK>
struct PairLoads {
    __amdgpu_buffer_rsrc_t rs;
    int off[PairSpan<R, EK>::NC];
};

template <int R, int EK = kF32>
__device__ __forceinline__ PairLoads<R, EK> plan_pair_loads(PairSpan<R, EK> &ps, const LookupArgs &a, int lo,
                                                              float x, long long pblk, long long lrow) {
    typedef PairSpan<R, EK> PS;
    int lo_e, hi_e;
    plan_pair<R, EK>(ps, a, lo, x, lo_e, hi_e);
    const int sa = 2 * ((int)ps.m - R - 1);
    const int ea = sa & ~(PS::EPC - 1);
    ps.sh = sa - ea;
    const long long ld = a.ld[lo];
    const char *lvl = static_cast<const char *>(a.lvl[lo]);
    // RC_SHADOW: the level also lies at +shb bytes, shifted by half a 128-B
    // line; each lane reads its span from the copy in which it touches fewer
    // lines (same values either way).  The resource then spans both copies.
    const long long shb = a.shadow[lo];
    PairLoads<R, EK> pl;
    pl.rs = make_rsrc(lvl + pblk * ld * PS::ES, clamp_bytes((a.P - pblk) * ld * PS::ES + shb));
    uint32_t phase = 0;
    if (shb != 0 && lo_e <= hi_e) {
        const unsigned long long b0 =
            (unsigned long long)(uintptr_t)(lvl + ((pblk + lrow) * ld + (lo_e & ~(PS::EPC - 1))) * PS::ES);
        const unsigned long long b1 = (unsigned long long)(uintptr_t)(lvl + ((pblk + lrow) * ld + hi_e) * PS::ES);
        const unsigned long long sh = (unsigned long long)shb;
        const long long l0 = (long long)(b1 >> 7) - (long long)(b0 >> 7);
        const long long l1 = (long long)((b1 + sh) >> 7) - (long long)((b0 + sh) >> 7);
        phase = l1 < l0 ? (uint32_t)sh : 0u;
    }
#pragma unroll
    for (int k = 0; k < PS::NC; ++k) {
        const int cs = ea + PS::EPC * k;
        // lo_e >= 0 and hi_e < Wlo: a loaded chunk starts inside the row and
        // ends inside its 16-B padded extent (ld % EPC == 0)
        const bool ok = cs <= hi_e && cs + PS::EPC - 1 >= lo_e;
        pl.off[k] = ok ? (int)((uint32_t)((lrow * ld + cs) * PS::ES) + phase) : (int)0xFFFFFF00u;
    }
    return pl;
}

template <int R, int EK>
__device__ __forceinline__ void load_pair(PairSpan<R, EK> &ps, const PairLoads<R, EK> &pl) {
#pragma unroll
    for (int k = 0; k < PairSpan<R, EK>::NC; ++k) {
        const auto v = __builtin_amdgcn_raw_buffer_load_b128(pl.rs, pl.off[k], 0, 0);
#pragma unroll
        for (int c = 0; c < 4; ++c) ps.q[k][c] = v[c];
    }
}

// Taps of one level from its zero-padded window w[NW] (element nwin-R-1+jj),
// the reference's fp32 sequence (see lookup_kernel).  No per-tap check that
// the tap's floor stayed in the window is needed here, because it cannot leave
// it: for a lane in the window's range (|xl| < W + R + 4) and W <= 2^16,
//  (1) xt = fl(xl + k) lies in [m, m + 1] with m = floor(xl) + k = nt
//      (integers are representable and rounding is monotone);
//  (2) the round trip xp = fl(fl(fl(fl(2 xt)/(W-1)) - 1) + 1) * (W-1)/2
//      differs from xt by at most (4|xt| + 1.5(W-1)) 2^-24 < 0.03;
// so x0 = floor(xp) is nt - 1, nt or nt + 1 (nt + 2 would need xt = nt + 1
// and an error >= 1), i.e. taps x0 and x0 + 1 are window elements t..t+3.
// The C-ABI rejects wider levels for this kernel (include/raftcorr.h).
// xa, xb: x' of taps -R and +R, which plan_pair has already evaluated for the
// exact span.
template <int R>
__device__ __forceinline__ void window_taps(const float *w, float xl, float nwin, const LevelConsts &lc,
                                            float xa, float xb, float *res) {
    constexpr int T = 2 * R + 1, NW = 2 * R + 4;
    // opaque copies: the selects must stay selects of registers (folded into
    // a load from a select of addresses, the window goes to scratch memory:
    // 112 B/lane and 87 instead of 14 vector loads per wave)
    float e[NW];
#pragma unroll
    for (int j = 0; j < NW; ++j) {
        e[j] = w[j];
        asm("" : "+v"(e[j]));
    }
#pragma unroll
    for (int t = 0; t < T; ++t) {
        const float xp = t == 0 ? xa : (t == T - 1 ? xb : tap_xp(xl, t - R, lc));
        const float x0 = floorf(xp);
        const float w1 = xp - x0, w0 = 1.0f - w1;
        const float nt = nwin + (float)(t - R);
        const bool lo_ = x0 < nt, hi_ = x0 > nt;
        const float v0 = lo_ ? e[t] : (hi_ ? e[t + 2] : e[t + 1]);
        const float v1 = lo_ ? e[t + 1] : (hi_ ? e[t + 3] : e[t + 2]);
        res[t] = fmaf(w1, v1, w0 * v0);
    }
}

// The memory path for a lane whose level pair breaks the span relation
// n = 2m + dd (only a subnormal x can): every tap re-read, level-i element k
// = pool of S consecutive span-level elements.
// level-i element k (S consecutive 16-bit span-level elements of kind EK,
// each level of the chain rounded to that kind as stored)
template <int S, int EK>
__device__ __forceinline__ float derived_elem_h16(const uint16_t *row, long long k) {
    if constexpr (S == 1) {
        return h16_to_f32(row[k], EK);
    } else {
        const float a = derived_elem_h16<S / 2, EK>(row, 2 * k), b = derived_elem_h16<S / 2, EK>(row, 2 * k + 1);
        return round_h16((a + b) * 0.5f, EK);
    }
}

template <int R, int S, int EK = kF32>
__device__ __forceinline__ void level_taps_mem(const void *rowv, float xl, const LevelConsts &lc, float *res) {
    constexpr int T = 2 * R + 1;
    const float Wm1 = lc.Wm1;
    for (int t = 0; t < T; ++t) {
        const float xp = tap_xp(xl, t - R, lc);
        const float x0 = floorf(xp);
        const float w1 = xp - x0, w0 = 1.0f - w1;
        const bool ok0 = (x0 >= 0.0f) && (x0 <= Wm1);
        const bool ok1 = (x0 + 1.0f >= 0.0f) && (x0 + 1.0f <= Wm1);
        float v0 = 0.0f, v1 = 0.0f;
        if constexpr (EK != kF32) {
            const uint16_t *row = static_cast<const uint16_t *>(rowv);
            if (ok0) v0 = derived_elem_h16<S, EK>(row, (long long)x0);
            if (ok1) v1 = derived_elem_h16<S, EK>(row, (long long)x0 + 1);
        } else {
            const float *row = static_cast<const float *>(rowv);
            if (ok0) v0 = derived_elem<S>(row, (long long)x0);
            if (ok1) v1 = derived_elem<S>(row, (long long)x0 + 1);
        }
        res[t] = fmaf(w1, v1, w0 * v0);
    }
}

// The span's elements from its loaded chunks: span element j = chunk element
// j + sh, sh in {0, 2, .., EPC-2}.  This consumes the chunks: after it their
// registers are free for the next span's loads.
template <int R, int EK>
__device__ __forceinline__ void span_shift(const PairSpan<R, EK> &ps, float *s) {
    typedef PairSpan<R, EK> PS;
#pragma unroll
    for (int j = 0; j < PS::NS; ++j) {
        float v = ps.elem(j);
#pragma unroll
        for (int d = 2; d < PS::EPC; d += 2)
            if (j + d < PS::NC * PS::EPC) v = (ps.sh == d) ? ps.elem(j + d) : v;
        s[j] = v;
    }
}

// Both levels of a pair from its span s[NS]: the two windows (after which
// the span is dead), then the even level's taps and stores, then the odd
// level's, so that one level's x' and results are live at a time.
template <int R, bool NOFALLBACK = false, int EK = kF32, class Sink, class Mid>
__device__ __forceinline__ void finish_span(const PairSpan<R, EK> &ps, const float *s, const LookupArgs &a,
                                            int lo, float x, long long pp, Sink &&sink, Mid &&mid) {
    typedef PairSpan<R, EK> PS;
    constexpr int T = 2 * R + 1, NW = PS::NW;
    const int Wlo = a.W[lo], Whi = a.W[lo + 1];
    const int mi = (int)ps.m - R - 1, ni = (int)ps.n - R - 1;
    const int dd = (int)ps.n - 2 * (int)ps.m;
    const float xlo = x / (float)(1 << lo), xhi = x / (float)(2 << lo);
    const bool mem = !NOFALLBACK && ps.inwin && !ps.valid;            // subnormal x only
    const char *row = static_cast<const char *>(a.lvl[lo]) + pp * a.ld[lo] * PS::ES;
    float weven[NW], wodd[NW];
#pragma unroll
    for (int jj = 0; jj < NW; ++jj) {
        float pm = (s[2 * jj] + s[2 * jj + 1]) * 0.5f;      // model.py:294 in fp32
        if constexpr (EK != kF32) pm = round_h16(pm, EK);  // the odd level as stored
        wodd[jj] = (unsigned)(mi + jj) < (unsigned)Whi ? pm : 0.0f;
        const float e = dd == 0 ? s[R + 1 + jj] : s[R + 2 + jj];
        weven[jj] = (unsigned)(ni + jj) < (unsigned)Wlo ? e : 0.0f;
    }
    const LevelConsts clo = level_consts(a, lo), chi = level_consts(a, lo + 1);
    float r[T];
    window_taps<R>(weven, xlo, ps.n, clo, ps.xe[0], ps.xe[1], r);
    if (__builtin_expect(mem, 0)) level_taps_mem<R, 1, EK>(row, xlo, clo, r);
#pragma unroll
    for (int t = 0; t < T; ++t) sink(lo * T + t, r[t]);
    mid();
    window_taps<R>(wodd, xhi, ps.m, chi, ps.xe[2], ps.xe[3], r);
    if (__builtin_expect(mem, 0)) level_taps_mem<R, 2, EK>(row, xhi, chi, r);
#pragma unroll
    for (int t = 0; t < T; ++t) sink((lo + 1) * T + t, r[t]);
}

template <int R, bool NOFALLBACK = false, int EK = kF32, class Sink>
__device__ __forceinline__ void finish_pair(const PairSpan<R, EK> &ps, const LookupArgs &a, int lo,
                                            float x, long long pp, Sink &&sink) {
    float s[PairSpan<R, EK>::NS];
    span_shift<R, EK>(ps, s);
    finish_span<R, NOFALLBACK, EK>(ps, s, a, lo, x, pp, sink, [] {});
}

// One lane's pixel of one group: index, x, output offset (elements of a.out,
// whatever their type: channel 0 of the NCHW output), rsrc base row.  Kept
// independent of the kernels' output type OT: with q type-dependent, the
// records kernel's buffer_load ... lds builtin is checked on instantiation in
// the host pass too, which then drops the kernel's launch stub without a word.
struct PairPixel {
    long long pblk, pp, lrow;
    long long ooff;
    float x;
    bool active;
};

template <int R, int NL>
__device__ __forceinline__ PairPixel pair_pixel(const LookupArgs &a, long long pblk) {
    PairPixel q;
    q.pblk = pblk;
    const long long p = pblk + threadIdx.x;
    q.active = p < a.P;
    q.pp = q.active ? p : a.P - 1;
    const long long bimg = q.pp / a.HW, rem = q.pp - bimg * a.HW;
    q.x = pixel_x(a, bimg, rem, q.active);
    q.ooff = bimg * (long long)(NL * (2 * R + 1)) * a.HW + rem;
    q.lrow = q.pp - pblk;
    return q;
}

// NL = 2 (levels 0-1) or 4 (levels 0-3; level 2 stored, levels 1 and 3 derived).
// Load schedule (pinned with sched_barrier): span 0's 7
// loads; span 2's address math while they are in flight; span 0's chunks
// shifted into its span; level 0's taps and stores; span 2's 7 loads, into
// the registers span 0's chunks held; level 1's taps and stores while those
// are in flight; then levels 2 and 3.  A wave makes two round trips of 7
// loads, not one of 14: with all 14 issued first (or span 2's right after
// the shift) the kernel needs 140-144 VGPRs, three waves per SIMD instead of
// four, and is slower (25.0 / 25.2 us against 22.7).  Left to the compiler,
// span 2's loads sank below both levels of span 0 (24.0 us).
// Measured and not kept: 16-B output
// stores through a per-wave LDS tile (9 instead of 36 store instructions per
// wave: 26.0 vs 25.8 us), two pixels per lane with both pixels' loads in
// flight (26.6 us, 198 VGPRs).
// M: ablation modes (dev library only, dev/lookup_dev.inc): 1 = no output
// stores, 2 = no fallback path, 5 = hardware block order (no XCD remap; same
// values), 7 = non-temporal output stores, 9 = the channels-last store path
// writing into an NCHW buffer (timing A/B of the two layouts); WPE caps
// registers for 5/6 waves/SIMD.
// OT: output element (float; _Float16 / __bf16 for RC_OUT_F16 / RC_OUT_BF16,
// instantiated in lookup_half.hip).  Only the sink and the channels-last tile
// depend on it: the fp32 value that is rounded is the fp32 kernel's.  NCHW:
// one 2-byte store per lane and channel plane (a 128-B run per wave; plane
// bases are only 2-byte aligned when H*W1 is odd, so nothing wider).
// The kernel's body is lookup_pair_body (EK: the pyramid's element kind):
// lookup_pair_kernel wraps it for fp32 and bf16 pyramids, lookup_f16pyr.hip
// for fp16 ones under a name of its own.
template <int R, int NL, int M, int EK, bool CL, class OT>
__device__ __forceinline__ void lookup_pair_body(const LookupArgs &a) {
    static_assert(NL == 2 || NL == 4, "pair lookup: 2 or 4 levels");
    constexpr int NP = NL / 2;                        // spans per pixel
    // XCD-contiguous block order: neighbouring pixel blocks, whose output
    // rows share 128-B lines at every channel plane's seams, run on one XCD
    // (kitti B=64: 172 -> 166 us; config 2 unchanged; dev variant 205 = off)
    const int blk = M == 5 ? (int)blockIdx.x : xcd_remap(blockIdx.x, gridDim.x);
    const PairPixel q = pair_pixel<R, NL>(a, (long long)blk * 256);
    OT *const outp = reinterpret_cast<OT *>(a.out) + q.ooff;
    PairSpan<R, EK> sp[NP];
    // The load schedule, pinned: the first span's loads go
    // out before the second span's address math; the second span's loads go
    // out between the two levels of the first (see below).
    PairLoads<R, EK> pl[NP];
    pl[0] = plan_pair_loads<R, EK>(sp[0], a, 0, q.x, q.pblk, q.lrow);
    load_pair<R, EK>(sp[0], pl[0]);
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (NP > 1) pl[1] = plan_pair_loads<R, EK>(sp[1], a, 2, q.x, q.pblk, q.lrow);
    constexpr int C = NL * (2 * R + 1);
    // CL: channels-last output (RC_OUT_CHANNELS_LAST), out[p*C + ch].  A
    // wave's 64 pixels own one contiguous run of 64*C elements; it is gathered
    // in a per-wave LDS tile and written as 16-B vectors, 1 KB per store
    // instruction (instead of C dword stores, 256 B each, to C channel planes)
    constexpr bool TILE = CL || M == 9;
    __shared__ __attribute__((aligned(16))) OT ctile[TILE ? 4 * 64 * C : 1];
    auto sink = [&](int ch, float v) {
        if constexpr (TILE) {
            ctile[(threadIdx.x >> 6) * 64 * C + (threadIdx.x & 63) * C + ch] = out_cvt<OT>(v);
        } else if constexpr (M == 7) {        // dev: non-temporal output stores
            if (q.active) __builtin_nontemporal_store(v, outp + (long long)ch * a.HW);
        } else {
            if (q.active && (M != 1 || v == 1234.5f)) outp[(long long)ch * a.HW] = out_cvt<OT>(v);
        }
    };
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        float s[PairSpan<R, EK>::NS];
        span_shift<R, EK>(sp[k], s);
        // The next span's loads: after this span's even level is done and
        // stored, before its odd level.  By then the shift has consumed this
        // span's chunks and the even level's window and x' are dead, so the
        // 28 registers the loads land in fit under 128 VGPRs (4 waves per
        // SIMD: the one-round grid); right after the shift they do not (140).
        // The scheduler may move nothing across the barriers.
        auto next = [&] {
            if constexpr (NP > 1) {
                if (k == 0) {
                    __builtin_amdgcn_sched_barrier(0);
                    load_pair<R, EK>(sp[1], pl[1]);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        };
        finish_span<R, M == 2, EK>(sp[k], s, a, 2 * k, q.x, q.pp, sink, next);
        __builtin_amdgcn_sched_barrier(0);
    }
    if constexpr (TILE) {
        // the wave's tile is private and LDS runs a wave's operations in
        // order: no barrier.  The run starts 64*C*sizeof(OT)-byte aligned.
        // Its valid length is a multiple of C, not of EPV: the last vector of
        // a partial wave goes out element by element.
        constexpr int EPV = 16 / (int)sizeof(OT);     // elements per 16-B vector (C is even: 64*C % EPV == 0)
        typedef OT ovec __attribute__((ext_vector_type(EPV)));
        const int lane = threadIdx.x & 63;
        const long long pw = q.pblk + (threadIdx.x & ~63);
        const OT *t = ctile + (threadIdx.x >> 6) * 64 * C;
        OT *const outb = reinterpret_cast<OT *>(a.out);
        const long long lim = (a.P - pw < 64 ? a.P - pw : 64) * C;   // valid elements of the run
#pragma unroll
        for (int k = 0; k < (64 * C / EPV + 63) / 64; ++k) {
            const int e = (k * 64 + lane) * EPV;           // element of the wave's [64][C] run
            if (e >= 64 * C || e >= lim) continue;
            const ovec v = *reinterpret_cast<const ovec *>(t + e);
            if (e + EPV <= lim) {
                *reinterpret_cast<ovec *>(outb + pw * C + e) = v;
            } else {
#pragma unroll
                for (int j = 0; j < EPV; ++j)
                    if (e + j < lim) outb[pw * C + e + j] = v[j];
            }
        }
    }
}

template <int R, int NL, int M = 0, bool BF16 = false, int WPE = 1, bool CL = false, class OT = float>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(WPE))) void lookup_pair_kernel(LookupArgs a) {
    lookup_pair_body<R, NL, M, BF16 ? kBF16 : kF32, CL, OT>(a);
}

// finish_pair's memory path over the disparity-major layout: every tap of
// level lo (stored) and lo + 1 (its pairwise means) re-read, the fp32 ops of
// level_taps_mem.
template <int R, class Sink>
__device__ __forceinline__ void sheared_taps_mem(const LookupArgs &a, int lo, float x, long long bh, int w1,
                                                 Sink &&sink) {
    constexpr int T = 2 * R + 1;
    const float *S = static_cast<const float *>(a.lvl[lo]) + bh * a.shk[lo] * a.ld[lo];
    const int W0 = a.W[lo];
    const long long base = (long long)((w1 >> lo) + W0 - 1);        // row of element 0 is base - j
    auto elem = [&](long long j) { return S[(base - j) * a.ld[lo] + w1]; };
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const LevelConsts lc = level_consts(a, lo + half);
        const float Wm1 = lc.Wm1;
        const float xl = x / (float)(1 << (lo + half));
        for (int t = 0; t < T; ++t) {
            const float xp = tap_xp(xl, t - R, lc);
            const float x0 = floorf(xp);
            const float wt1 = xp - x0, wt0 = 1.0f - wt1;
            const bool ok0 = (x0 >= 0.0f) && (x0 <= Wm1);
            const bool ok1 = (x0 + 1.0f >= 0.0f) && (x0 + 1.0f <= Wm1);
            const long long e = (long long)x0;
            float v0 = 0.0f, v1 = 0.0f;
            if (half == 0) {
                if (ok0) v0 = elem(e);
                if (ok1) v1 = elem(e + 1);
            } else {
                if (ok0) v0 = (elem(2 * e) + elem(2 * e + 1)) * 0.5f;
                if (ok1) v1 = (elem(2 * e + 2) + elem(2 * e + 3)) * 0.5f;
            }
            sink((lo + half) * T + t, fmaf(wt1, v1, wt0 * v0));
        }
    }
}

// ---- lookup over a disparity-major pair layout (RC_LAYOUT_DISPARITY) ----
// The pair kernel's arithmetic (levels 0 and 2 stored, 1 and 3 their
// pairwise means, finish_pair: bit-identical) over levels stored as
// S_i[b,h][k][w1], k = (w1 >> i) - j + W_i - 1 (rc_corr_build with the
// flag; a.shk[i] rows of a.ld[i] floats per image row): the lanes of a wave
// whose pixels look at the same disparity read one contiguous run of a row
// per span element -- coalesced along w1 -- instead of a 16-B piece of 64
// different pixel rows.  A span is 2(2r+4) dword loads per lane (exact-span
// predicated).  Faster than the row layout where neighbouring pixels' coords
// agree (the network's own fields), slower on independent random ones
// (DESIGN.md §3.2h).
template <int R, int NL>
__global__ __launch_bounds__(256) void lookup_sheared_pair_kernel(LookupArgs a) {
    static_assert(NL == 2 || NL == 4, "pair lookup: 2 or 4 levels");
    constexpr int NP = NL / 2, NS = PairSpan<R>::NS;
    const int blk = xcd_remap(blockIdx.x, gridDim.x);
    const long long pblk = (long long)blk * 256;
    const long long p = pblk + threadIdx.x;
    const bool active = p < a.P;
    const long long pp = active ? p : a.P - 1;
    const long long bimg = pp / a.HW, rem = pp - bimg * a.HW;
    const float x = pixel_x(a, bimg, rem, active);
    const int H = a.HW / a.W1;
    const int h = (int)(rem / a.W1), w1 = (int)(rem - (long long)h * a.W1);
    const long long bh = bimg * H + h, bh0 = pblk / a.W1;          // bh0: block-uniform
    float *outp = a.out + bimg * (long long)(NL * (2 * R + 1)) * a.HW + rem;
    auto sink = [&](int ch, float v) {
        if (active) outp[(long long)ch * a.HW] = v;
    };
    PairSpan<R> sp[NP];
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        const int lo = 2 * k;
        PairSpan<R> &ps = sp[k];
        const int Wlo = a.W[lo];
        int lo_e, hi_e;
        plan_pair<R, false>(ps, a, lo, x, lo_e, hi_e);
        ps.sh = 0;
        const int sa = 2 * ((int)ps.m - R - 1);
        const long long K = a.shk[lo], ldw = a.ld[lo];
        const float *lv = static_cast<const float *>(a.lvl[lo]);
        const auto rs = make_rsrc(lv + bh0 * K * ldw, clamp_bytes((a.P / a.W1 - bh0) * K * ldw * 4));
        const long long rowk = (bh - bh0) * K + (w1 >> lo) + Wlo - 1;    // row of element 0
#pragma unroll
        for (int c = 0; c < PairSpan<R>::NC * 4; ++c) {
            const int j = sa + c;
            const bool ok = c < NS && j >= lo_e && j <= hi_e;
            const uint32_t off = ok ? (uint32_t)(((rowk - j) * ldw + w1) * 4) : 0xFFFFFF00u;
            ps.q[c >> 2][c & 3] = __builtin_amdgcn_raw_buffer_load_b32(rs, (int)off, 0, 0);
        }
    }
    // a subnormal x (the only way to break n = 2m + dd) takes the memory path
    // of finish_pair, which reads the row layout: not available here, so the
    // taps of such a lane come from sheared_taps_mem below instead
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        if (__builtin_expect(sp[k].inwin && !sp[k].valid, 0)) {
            sheared_taps_mem<R>(a, 2 * k, x, bh, w1, sink);
            continue;
        }
        finish_pair<R, true>(sp[k], a, 2 * k, x, pp, sink);
    }
}

// ---- lookup over the record layout (RC_LAYOUT_RECORDS, bf16, 4 levels) ----
// Each pixel row holds a.rec_nr 128-B records (rc_corr_build with the flag;
// geometry in common.h): record r has level-2 elements rec_e2(r) .. +25 in
// slots 0..25 and level-0 elements rec_e0(r) .. +37 in slots 26..63, so a
// pixel whose level-1 centre m1 = floor(x/2) lies in [8r - 8, 8r) finds both
// of its pair spans (level 0's from 2(m1 - R - 1), level 2's from
// 2(floor(m1/4) - R - 1)) in record r: ONE 128-B line per pixel instead of
// two.  A pixel outside the records' m1 range takes the
// nearest record; its exact spans are then empty or lie at the row edge that
// record covers.  The chunks are read with plan_pair's exact-span predicate
// and finish_pair runs unchanged, so the output is the row layout's bit for
// bit.

// plan_pair_loads / load_pair over a record: level-lo element e sits in slot e - e_first + slot_first.
// plan_record_pair fills the span's window fields and returns the first
// chunk's slot (cb, a multiple of 8) and which of the NC chunks the taps read.
template <int R>
__device__ __forceinline__ int plan_record_pair(PairSpan<R, true> &ps, const LookupArgs &a, int lo, float x,
                                                int e_first, int slot_first, uint32_t &okmask) {
    typedef PairSpan<R, true> PS;
    int lo_e, hi_e;
    plan_pair<R, true>(ps, a, lo, x, lo_e, hi_e);
    const int sslot = 2 * ((int)ps.m - R - 1) - e_first + slot_first;   // span start (even)
    const int cb = sslot >= 0 ? sslot & ~7 : -((-sslot + 7) & ~7);      // chunk base (floor to 8)
    ps.sh = sslot - cb;
    const int slo = lo_e - e_first + slot_first, shi = hi_e - e_first + slot_first;
    okmask = 0;
#pragma unroll
    for (int k = 0; k < PS::NC; ++k) {
        const int cs = cb + 8 * k;
        if (lo_e <= hi_e && cs <= shi && cs + 7 >= slo && cs >= 0 && cs + 8 <= kRecSlots) okmask |= 1u << k;
    }
    return cb;
}

template <int R, bool NOLOAD = false>
__device__ __forceinline__ void issue_record_pair(PairSpan<R, true> &ps, const LookupArgs &a, int lo, float x,
                                                  const __amdgpu_buffer_rsrc_t &rs, uint32_t rbyte, int e_first,
                                                  int slot_first) {
    typedef PairSpan<R, true> PS;
    uint32_t okm;
    const int cb = plan_record_pair<R>(ps, a, lo, x, e_first, slot_first, okm);
#pragma unroll
    for (int k = 0; k < PS::NC; ++k) {
        const int cs = cb + 8 * k;
        const bool ok = (okm >> k) & 1u;
        if constexpr (NOLOAD) {   // dev timing: the addresses, not the loads
            uint32_t o = ok ? rbyte + 2u * (uint32_t)cs : 0u;
            asm volatile("" : "+v"(o));
#pragma unroll
            for (int c = 0; c < 4; ++c) ps.q[k][c] = o + c;
        } else {
            const auto v = __builtin_amdgcn_raw_buffer_load_b128(
                rs, ok ? (int)(rbyte + 2u * (uint32_t)cs) : (int)0xFFFFFF00u, 0, 0);
#pragma unroll
            for (int c = 0; c < 4; ++c) ps.q[k][c] = v[c];
        }
    }
}

// The same chunks from the pixel's whole record staged in LDS (COOP).
template <int R>
__device__ __forceinline__ void lds_record_pair(PairSpan<R, true> &ps, const LookupArgs &a, int lo, float x,
                                                const char *rec, int e_first, int slot_first) {
    typedef PairSpan<R, true> PS;
    uint32_t okm;
    const int cb = plan_record_pair<R>(ps, a, lo, x, e_first, slot_first, okm);
#pragma unroll
    for (int k = 0; k < PS::NC; ++k) {
        const int cs = cb + 8 * k;
        uint4 v = uint4{0u, 0u, 0u, 0u};
        if ((okm >> k) & 1u) v = *reinterpret_cast<const uint4 *>(rec + 2 * cs);
        ps.q[k][0] = v.x;
        ps.q[k][1] = v.y;
        ps.q[k][2] = v.z;
        ps.q[k][3] = v.w;
    }
}

// finish_pair's memory path over the records (a subnormal x, the only way to
// break n = 2m + dd): level lo (0 or 2) element e from a record that holds
// it, level lo + 1 the bf16-rounded pairwise mean, the ops of level_taps_mem
template <int R, class Sink>
__device__ __forceinline__ void record_taps_mem(const LookupArgs &a, const uint16_t *rec, int lo, float x,
                                                Sink &&sink) {
    constexpr int T = 2 * R + 1;
    const int NR = a.rec_nr;
    auto elem = [&](long long e) {
        int r = lo == 0 ? (int)((e - rec_e0(0)) >> 4) : (int)((e - rec_e2(0)) >> 2);
        r = r < NR ? r : NR - 1;
        const int slot = lo == 0 ? kRecL2Slots + (int)e - rec_e0(r) : (int)e - rec_e2(r);
        return bf16_to_f32(rec[r * kRecSlots + slot]);
    };
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const LevelConsts lc = level_consts(a, lo + half);
        const float Wm1 = lc.Wm1;
        const float xl = x / (float)(1 << (lo + half));
        for (int t = 0; t < T; ++t) {
            const float xp = tap_xp(xl, t - R, lc);
            const float x0 = floorf(xp);
            const float wt1 = xp - x0, wt0 = 1.0f - wt1;
            const bool ok0 = (x0 >= 0.0f) && (x0 <= Wm1);
            const bool ok1 = (x0 + 1.0f >= 0.0f) && (x0 + 1.0f <= Wm1);
            const long long e = (long long)x0;
            float v0 = 0.0f, v1 = 0.0f;
            if (half == 0) {
                if (ok0) v0 = elem(e);
                if (ok1) v1 = elem(e + 1);
            } else {
                if (ok0) v0 = round_bf16((elem(2 * e) + elem(2 * e + 1)) * 0.5f);
                if (ok1) v1 = round_bf16((elem(2 * e + 2) + elem(2 * e + 3)) * 0.5f);
            }
            sink((lo + half) * T + t, fmaf(wt1, v1, wt0 * v0));
        }
    }
}

// CL: channels-last output (RC_OUT_CHANNELS_LAST) through the per-wave LDS
// tile of lookup_pair_kernel; else NCHW dword stores.  COOP (the product)
// see below; without it each lane loads its own chunks (the dev A/B).  M: dev timing modes
// (libraftcorr_dev.so, wrong output): 1 no output stores, 2 no record loads,
// 3 record loads only (no tap math, no stores).
// COOP: each wave's 64 records are fetched whole, eight 128-B lines per
// buffer_load ... lds instruction (lane L: record 8k + L/8, 16-B chunk L % 8)
// into a per-wave LDS image, then each lane reads its chunks from there:
// 8 line requests per instruction instead of 64 partial ones.
// OT: output element as in lookup_pair_kernel; with CL the tile holds OT
// elements (64 C sizeof(OT) bytes) and still aliases the staged records.
template <int R, bool CL, int M = 0, bool COOP = false, int WPE = 1, class OT = float>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(WPE))) void lookup_records_kernel(LookupArgs a) {
    constexpr int NL = 4, C = NL * (2 * R + 1);
    const int blk = xcd_remap(blockIdx.x, gridDim.x);
    const PairPixel q = pair_pixel<R, NL>(a, (long long)blk * 256);
    const int NR = a.rec_nr;
    // the pixel's record (clamped as floats before the integer cast: NaN -> 0)
    float mf = floorf(q.x / 2.0f);
    mf = fminf(fmaxf(mf, (float)kRecM0), (float)(kRecM0 + 8 * NR - 1));
    const int r = ((int)mf - kRecM0) >> 3;
    const uint16_t *blkrec = static_cast<const uint16_t *>(a.lvl[0]) + q.pblk * (long long)NR * kRecSlots;
    // the block's records (< 4 GiB: 256 rows of <= 22 lines)
    const auto rs = make_rsrc(blkrec, clamp_bytes((a.P - q.pblk) * (long long)NR * kRecSlots * 2));
    const uint32_t rbyte = (uint32_t)((q.lrow * NR + r) * kRecSlots * 2);
    PairSpan<R, true> sp[2];
    // per wave: the staged records (8 KB), then the channels-last tile
    // (64 C elements, 9 KB of floats at R = 4) in the same bytes once they are read
    constexpr int TB = 64 * C * (int)sizeof(OT);
    constexpr int WB = CL ? (COOP && TB < 8192 ? 8192 : TB) : (COOP ? 8192 : 16);
    __shared__ __attribute__((aligned(16))) char lds[4 * WB];
    char *wlds = lds + (threadIdx.x >> 6) * WB;
    if constexpr (COOP) {
        typedef __attribute__((address_space(3))) void lds_void;
        const int lane = threadIdx.x & 63;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            // record of pixel 8k + lane/8 of this wave, its chunk lane % 8
            const uint32_t rb = (uint32_t)__shfl((int)rbyte, 8 * k + (lane >> 3), 64);
            const int wp = (int)(threadIdx.x & ~63) + 8 * k + (lane >> 3);
            const uint32_t off = q.pblk + wp < a.P ? rb + 16u * (uint32_t)(lane & 7) : 0xFFFFFF00u;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_void *)(wlds + 1024 * k), 16, (int)off, 0, 0, 0);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const char *myrec = wlds + 128 * lane;
        lds_record_pair<R>(sp[0], a, 0, q.x, myrec, rec_e0(r), kRecL2Slots);
        lds_record_pair<R>(sp[1], a, 2, q.x, myrec, rec_e2(r), 0);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // all reads done before the tile reuses the bytes
    } else {
        issue_record_pair<R, M == 2>(sp[0], a, 0, q.x, rs, rbyte, rec_e0(r), kRecL2Slots);
        issue_record_pair<R, M == 2>(sp[1], a, 2, q.x, rs, rbyte, rec_e2(r), 0);
    }
    if constexpr (M == 3) {   // dev: the loads alone
        uint32_t acc = 0;
#pragma unroll
        for (int k = 0; k < 2; ++k)
#pragma unroll
            for (int j = 0; j < PairSpan<R, true>::NC; ++j) acc ^= sp[k].q[j][0] ^ sp[k].q[j][1] ^ sp[k].q[j][2] ^ sp[k].q[j][3];
        asm volatile("" ::"v"(acc));
        return;
    }
    OT *const ctw = reinterpret_cast<OT *>(wlds);             // this wave's channels-last tile
    OT *const outp = reinterpret_cast<OT *>(a.out) + q.ooff;
    auto sink = [&](int ch, float v) {
        if constexpr (CL) ctw[(threadIdx.x & 63) * C + ch] = out_cvt<OT>(v);
        else if (q.active) outp[(long long)ch * a.HW] = out_cvt<OT>(v);
    };
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        if (__builtin_expect(sp[k].inwin && !sp[k].valid, 0)) {
            record_taps_mem<R>(a, blkrec + q.lrow * (long long)NR * kRecSlots, 2 * k, q.x, sink);
            continue;
        }
        finish_pair<R, true, true>(sp[k], a, 2 * k, q.x, q.pp, sink);
    }
    if constexpr (CL) {
        const int lane = threadIdx.x & 63;
        const long long pw = q.pblk + (threadIdx.x & ~63);
        constexpr int EPV = 16 / (int)sizeof(OT);         // as in lookup_pair_kernel
        typedef OT ovec __attribute__((ext_vector_type(EPV)));
        const OT *t = ctw;
        OT *const outb = reinterpret_cast<OT *>(a.out);
        const long long lim = (a.P - pw < 64 ? a.P - pw : 64) * C;
#pragma unroll
        for (int k = 0; k < (64 * C / EPV + 63) / 64; ++k) {
            const int e = (k * 64 + lane) * EPV;
            if (e >= 64 * C || e >= lim) continue;
            const ovec v = *reinterpret_cast<const ovec *>(t + e);
            if constexpr (M == 1) {   // dev: no output stores
                asm volatile("" ::"v"(v));
            } else if (e + EPV <= lim) {
                *reinterpret_cast<ovec *>(outb + pw * C + e) = v;
            } else {
#pragma unroll
                for (int j = 0; j < EPV; ++j)
                    if (e + j < lim) outb[pw * C + e + j] = v[j];
            }
        }
    }
}

}  // namespace rc
