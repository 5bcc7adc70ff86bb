// Radius-r lookup over the correlation pyramid (gfx950).
//
// Replaces CorrBlock1D.__call__ (/root/reference/model.py:297-316) and the
// grid_sample-based bilinear_sampler it calls (:267-281).  For pixel p =
// (b,h,w1), level i and tap t in -r..r the reference samples row p of level i at
//     x_t = t + x/2^i                                          (:305-307)
//     xn  = 2*x_t/(W_i-1) - 1                                  (:271)
//     x'  = (xn + 1) * ((W_i-1)/2)      grid_sample, align_corners=True (:275)
//     x0 = floor(x'), w1 = x' - x0, w0 = 1 - w1
//     out = fma(w1, v(x0+1), w0*v(x0)),  v(k) = 0 outside [0, W_i)   (zeros pad)
// and writes channel i*(2r+1)+t+r of a (B, L(2r+1), H, W1) fp32 tensor
// (:315-316).  The normalise/unnormalise round trip is kept bit-for-bit: it
// moves x' by up to ~1e-4 px at W=720.  The file is built with
// -ffp-contract=off so the only fused op is the explicit fmaf.
//
// Memory: one lane per pixel.  The taps of one level touch the elements
// [x0_first, x0_last + 1] (x0 is monotone in t), which lie inside the 2r+4
// element window [n-r-1, n+r+2] (n = floor(x/2^i)) because the round trip
// moves floor(x') by at most one.  The lane fetches that window with 16-byte
// buffer loads aligned to the row start of the level; a load whose 16 bytes
// miss [x0_first, x0_last+1] gets an out-of-range offset instead, so it
// returns zeros and touches no memory (branch-free predication).  The window
// is shifted by its 0..3 (fp32) / 0..7 (bf16) misalignment with selects and
// each tap picks its pair with a 3-way select.  With the level count a
// template parameter, every level's loads issue before any tap math.  A tap
// whose floor is off by more than one (impossible for |x| < 2^22 by the error
// bound; kept for safety) takes a guarded scalar path.  Output stores are
// coalesced along w1.
#include <type_traits>

#include "common.h"
#include "lookup_level.h"   // pixel_x, LevelWindow, issue_level, finish_level
#include "lookup_pair.h"    // pool_tree, derived_elem; the pair / sheared pair / records kernels

namespace rc {

// NL > 0: compile-time level count (all loads issue first); NL == 0: runtime.
// BS = threads per block (256 for throughput, 64 to spread small problems).
template <int R, int NL, bool BF16, bool EXACT, int BS = 256, int WPE = 1>
__global__ __launch_bounds__(BS) __attribute__((amdgpu_waves_per_eu(WPE)))
void lookup_kernel(LookupArgs a) {
    constexpr int T = 2 * R + 1;
    const long long pblk = (long long)blockIdx.x * BS;
    const long long p = pblk + threadIdx.x;
    const bool active = p < a.P;
    const long long pp = active ? p : a.P - 1;
    const long long bimg = pp / a.HW, rem = pp - bimg * a.HW;
    const float x = pixel_x(a, bimg, rem, active);
    const int L = NL > 0 ? NL : a.levels;
    float *outp = a.out + bimg * (long long)(L * T) * a.HW + rem;
    const long long lrow = pp - pblk;
    if constexpr (NL > 0) {
        LevelWindow<R, BF16> lw[NL];
#pragma unroll
        for (int i = 0; i < NL; ++i) issue_level<R, BF16, EXACT>(lw[i], a, i, x, pblk, lrow);
#pragma unroll
        for (int i = 0; i < NL; ++i)
            finish_level<R, BF16>(lw[i], a, i, pblk, lrow, [&](int t, float v) {
                if (active) outp[(long long)(i * T + t) * a.HW] = v;
            });
    } else {
        for (int i = 0; i < L; ++i) {
            LevelWindow<R, BF16> lw;
            issue_level<R, BF16, EXACT>(lw, a, i, x, pblk, lrow);
            finish_level<R, BF16>(lw, a, i, pblk, lrow, [&](int t, float v) {
                if (active) outp[(long long)(i * T + t) * a.HW] = v;
            });
        }
    }
}

// Small problems (the realtime config: 19,200 pixels): a launch then lasts
// about one wave's chain of window loads and tap math, so a block gives each
// LEVEL its own wave -- wave i of block b looks up level i for pixels
// [64b, 64b+64) -- which shortens that chain ~L-fold.  Per level the code is
// lookup_kernel's (issue_level / finish_level): bit-identical results.  In
// the fused loop step every wave reads the pixel's coords before the block
// barrier and only wave 0 writes the advanced coords and flow after it (the
// outputs may alias coords1).
// XA: pixel blocks placed XCD by XCD (xcd_remap), so each XCD looks up one
// contiguous eighth of the rows -- the rows whose pyramid lines the build
// (xcd_remap'd by row) wrote through that XCD's L2.
template <int R, bool BF16, bool XA = true>
__global__ __launch_bounds__(256) void lookup_levelpar_kernel(LookupArgs a) {
    constexpr int T = 2 * R + 1;
    const int i = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));   // this wave's level
    const int blk = XA ? xcd_remap((int)blockIdx.x, (int)gridDim.x) : (int)blockIdx.x;
    const long long pblk = (long long)blk * 64;
    const long long p = pblk + (threadIdx.x & 63);
    const bool active = p < a.P;
    const long long pp = active ? p : a.P - 1;
    const long long bimg = pp / a.HW, rem = pp - bimg * a.HW;
    const float x = pixel_x(a, bimg, rem, false);
    if (a.step) {                                       // block-uniform
        __syncthreads();
        if (i == 0) (void)pixel_x(a, bimg, rem, active);
    }
    float *outp = a.out + bimg * (long long)(a.levels * T) * a.HW + rem;
    LevelWindow<R, BF16> lw;
    issue_level<R, BF16, true>(lw, a, i, x, pblk, pp - pblk);
    finish_level<R, BF16>(lw, a, i, pblk, pp - pblk, [&](int t, float v) {
        if (active) outp[(long long)(i * T + t) * a.HW] = v;
    });
}

// ---- lookup over a pool-chain pyramid: levels >= 2 derived from level 1 ----
// When the levels are the avg_pool chain of level 0 -- the pyramid
// rc_corr_build writes -- element j of level i >= 2 is the pairwise-mean tree
// of level-1 elements [2^(i-1) j, 2^(i-1) (j+1)) evaluated in the same fp32
// order as model.py:294 applied i-1 times, so it is recomputed from level 1
// bit for bit.  The windows of levels 1..L-1 around x all lie inside ONE span
// of level 1: the top level's 2r+4 window scaled by S = 2^(L-2) (48 elements
// at L = 4, r = 4), starting at a multiple of S.  Reading that span once
// (~2.1 128-B lines for its ~160-B exact part) replaces one ~1.3-line window
// per level, so a pixel touches ~3.4 lines instead of ~4.9.
// Level 0 keeps its own window.  fp32 pyramids only (a bf16 pyramid rounds
// every level separately).  pool_tree / derived_elem: lookup_pair.h.

// M: dev-only ablation (RAFTCORR_LOOKUP_VARIANT in launch_chain_r): 0 = product,
// 1 = no output stores (kept live by an impossible compare), 2 = no pyramid loads,
// 3 = pyramid loads only (no tap math, no stores), 4 = tap math only,
// 5 = the product with non-temporal output stores.
template <int R, int NL, int M = 0>
__global__ __launch_bounds__(256) void lookup_chain_kernel(LookupArgs a) {
    static_assert(NL >= 3 && NL <= 4, "chain lookup: 3 or 4 levels");
    constexpr int T = 2 * R + 1, NW = 2 * R + 4, TOP = NL - 1, S = 1 << (TOP - 1);
    constexpr int NE1 = S * NW;                        // span elements of level 1
    constexpr int SHM = (S % 4 == 0) ? 0 : 4 - S;      // max misalignment of its start
    constexpr int NC1 = (NE1 + SHM + 3) / 4;           // 16-B chunks
    const long long pblk = (long long)blockIdx.x * 256;
    const long long p = pblk + threadIdx.x;
    const bool active = p < a.P;
    const long long pp = active ? p : a.P - 1;
    const long long bimg = pp / a.HW, rem = pp - bimg * a.HW;
    const float x = pixel_x(a, bimg, rem, active);
    float *outp = a.out + bimg * (long long)(NL * T) * a.HW + rem;
    const long long lrow = pp - pblk;

    // level 0: its own window (lookup_kernel's path)
    LevelWindow<R, false> lw0;
    constexpr bool NOLOAD = M == 2 || M == 4, NOSTORE = M == 1 || M == 4;
    issue_level<R, false, true>(lw0, a, 0, NOLOAD ? NAN : x, pblk, lrow);

    // levels 1..TOP: one span of level 1, starting at e1 = S (n_top - R - 1)
    const float xtop = x / (float)(1 << TOP);
    const bool inwin = (xtop > -(float)(R + 4)) && (xtop < (float)(a.W[TOP] + R + 4));
    const float ntop = inwin ? floorf(xtop) : 0.0f;
    const int e1 = S * ((int)ntop - R - 1);
    const int ea = e1 & ~3;
    const int sh = e1 - ea;                            // 0 when S % 4 == 0
    int lo = 0x7FFFFFFF, hi = -1;                      // union of the exact spans
    if (inwin) {
#pragma unroll
        for (int i = 1; i <= TOP; ++i) {
            const float Wm1 = (float)(a.W[i] - 1), half = Wm1 / 2.0f;
            const DivRN dv = div_prep(Wm1);
            const float xl = x / (float)(1 << i);
            const float xa = (float)(-R) + xl, xb = (float)R + xl;
            const float pa = ((div_rn(2.0f * xa, dv) - 1.0f) + 1.0f) * half;
            const float pb = ((div_rn(2.0f * xb, dv) - 1.0f) + 1.0f) * half;
            const int f = max((int)floorf(pa), 0);
            const int l = min((int)floorf(pb) + 1, a.W[i] - 1);
            if (f <= l) {
                lo = min(lo, f << (i - 1));
                hi = max(hi, ((l + 1) << (i - 1)) - 1);
            }
        }
    }
    const long long ld1 = a.ld[1];
    const float *lvl1 = static_cast<const float *>(a.lvl[1]);
    const auto rs1 = make_rsrc(lvl1 + pblk * ld1, clamp_bytes((a.P - pblk) * ld1 * 4));
    f32x4 q1[NC1];
#pragma unroll
    for (int k = 0; k < NC1; ++k) {
        const int cs = ea + 4 * k;
        const bool ok = !NOLOAD && cs <= hi && cs + 3 >= lo;   // lo >= 0 and hi < W_1: inside the row
        q1[k] = ld4(rs1, ok ? (uint32_t)((lrow * ld1 + cs) * 4) : 0xFFFFFF00u);
    }
    if constexpr (M == 3) {
        uint32_t acc = 0;
#pragma unroll
        for (int k = 0; k < LevelWindow<R, false>::NV; ++k)
#pragma unroll
            for (int c = 0; c < 4; ++c) acc ^= lw0.q[k][c];
#pragma unroll
        for (int k = 0; k < NC1; ++k)
#pragma unroll
            for (int c = 0; c < 4; ++c) acc ^= __builtin_bit_cast(uint32_t, q1[k][c]);
        if (acc == 0x12345678u) outp[0] = 0.0f;
        return;
    }

    // level 0 math + stores while the span is in flight
    finish_level<R, false>(lw0, a, 0, pblk, lrow, [&](int t, float v) {
        if (!active) return;
        if constexpr (M == 5) __builtin_nontemporal_store(v, outp + (long long)t * a.HW);
        else if (!NOSTORE || v == 1234.5f) outp[(long long)t * a.HW] = v;
    });

    // s1[k] = level-1 element e1 + k
    float s1[NE1];
#pragma unroll
    for (int k = 0; k < NE1; ++k) {
        float r = q1[k >> 2][k & 3];
#pragma unroll
        for (int s = 1; s <= SHM; ++s)
            if (k + s < 4 * NC1) r = (sh == s) ? q1[(k + s) >> 2][(k + s) & 3] : r;
        s1[k] = r;
    }
    const float *row1 = lvl1 + pp * ld1;

    auto level = [&](auto ic) {
        constexpr int i = decltype(ic)::value;
        constexpr int SI = 1 << (i - 1), NDD = 1 << (TOP - i);
        const int W = a.W[i];
        const float Wm1 = (float)(W - 1), half = Wm1 / 2.0f;
        const DivRN dv = div_prep(Wm1);
        const float xl = x / (float)(1 << i);
        const float n = inwin ? floorf(xl) : 0.0f;
        // n = NDD * n_top + dd, dd in [0, NDD) (x / 2^i is exact); a subnormal
        // x can break that -- such a lane reads memory instead (valid = false)
        const int dd = inwin ? (int)n - NDD * (int)ntop : 0;
        const bool valid = inwin && dd >= 0 && dd < NDD;
        // window element jj (level-i element n - R - 1 + jj) starts at level-1
        // offset SI*(dd + jj) + (R+1)*(S - SI) of the span
        float w[NW];
#pragma unroll
        for (int jj = 0; jj < NW; ++jj) {
            float val = 0.0f;
#pragma unroll
            for (int d = 0; d < NDD; ++d) {
                constexpr int base = (R + 1) * (S - SI);
                const float v = pool_tree<SI>(s1 + base + SI * (d + jj));
                val = (dd == d) ? v : val;
            }
            w[jj] = val;
        }
        float res[T];
        bool bad = false;
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const float xt = (float)(t - R) + xl;
            const float xn = div_rn(2.0f * xt, dv) - 1.0f;
            const float xp = (xn + 1.0f) * half;
            const float x0 = floorf(xp);
            const float w1 = xp - x0, w0 = 1.0f - w1;
            const float nt = n + (float)(t - R);
            const bool lo_ = x0 < nt, hi_ = x0 > nt;
            const float a0 = lo_ ? w[t] : (hi_ ? w[t + 2] : w[t + 1]);
            const float a1 = lo_ ? w[t + 1] : (hi_ ? w[t + 3] : w[t + 2]);
            const bool ok0 = (x0 >= 0.0f) && (x0 <= Wm1);
            const bool ok1 = (x0 + 1.0f >= 0.0f) && (x0 + 1.0f <= Wm1);
            bad |= inwin && (!valid || x0 < nt - 1.0f || x0 > nt + 1.0f);
            const float v0 = ok0 ? a0 : 0.0f;
            const float v1 = ok1 ? a1 : 0.0f;
            res[t] = fmaf(w1, v1, w0 * v0);
        }
        if (__builtin_expect(bad, 0)) {   // one wave-level check per level
            for (int t = 0; t < T; ++t) {
                const float xt = (float)(t - R) + xl;
                const float xn = div_rn(2.0f * xt, dv) - 1.0f;
                const float xp = (xn + 1.0f) * half;
                const float x0 = floorf(xp);
                const float w1 = xp - x0, w0 = 1.0f - w1;
                const bool ok0 = (x0 >= 0.0f) && (x0 <= Wm1);
                const bool ok1 = (x0 + 1.0f >= 0.0f) && (x0 + 1.0f <= Wm1);
                const float v0 = ok0 ? derived_elem<SI>(row1, (long long)x0) : 0.0f;
                const float v1 = ok1 ? derived_elem<SI>(row1, (long long)x0 + 1) : 0.0f;
                res[t] = fmaf(w1, v1, w0 * v0);
            }
        }
        // inactive lanes (tail block) stand in for pixel P-1 and store nothing:
        // with rc_corr_lookup_step in place (coords_out == coords) they may have
        // read coords the real lane already advanced
        if (active) {
#pragma unroll
            for (int t = 0; t < T; ++t)
                if constexpr (M == 5) __builtin_nontemporal_store(res[t], outp + (long long)(i * T + t) * a.HW);
                else if (!NOSTORE || res[t] == 1234.5f) outp[(long long)(i * T + t) * a.HW] = res[t];
        }
    };
    level(std::integral_constant<int, 1>{});
    level(std::integral_constant<int, 2>{});
    if constexpr (TOP >= 3) level(std::integral_constant<int, 3>{});
}

// The pair-layout kernels (pair, disparity-major pair, records): lookup_pair.h.


template <int R, int NL, bool BF16, bool EXACT, int BS = 256, int WPE = 1>
static void launch_k(const LookupArgs &a, hipStream_t s) {
    const unsigned nblk = (unsigned)((a.P + BS - 1) / BS);
    hipLaunchKernelGGL((lookup_kernel<R, NL, BF16, EXACT, BS, WPE>), dim3(nblk), dim3(BS), 0, s, a);
}

// Below this many pixels the launch cannot fill the chip with the 256-thread
// runtime-loop kernel (one dependent memory round trip per level): use
// 64-thread blocks and issue every level's loads up front instead.
constexpr long long kSmallP = 256LL * 256 * 2;
// Below this many pixels one wave per (64 pixels, level) still leaves the
// chip under-filled or about full: lookup_levelpar_kernel.
constexpr long long kLevelParP = 64LL * 1024;

// ---- lookup fused with the motion encoder's convc1 (+ ReLU) ----
// BasicMotionEncoder.convc1 (model.py:199, :206) is a 1x1 conv over the
// lookup's NL*(2r+1) channels: out[c] = relu(bias[c] + sum_k W[c][k] corr[k]).
// The lane keeps its pixel's corr values in registers (levels unrolled, so
// every index is static) and never writes them; the weights are read with
// wave-uniform addresses (scalar loads).  Summation order: bias, then k
// ascending, one fmaf each.
// PRE (default): every level's loads issue before any tap math (NL windows
// live at once) instead of one level's round trip at a time: 52.9 vs 57.5 us
// at config 2, bit-identical.
template <int R, int NL, bool BF16, bool PRE = true>
__global__ __launch_bounds__(256) void lookup_conv_kernel(LookupArgs a, const float *__restrict__ wgt,
                                                          const float *__restrict__ bias, int cout,
                                                          int relu, float *__restrict__ out) {
    constexpr int T = 2 * R + 1, CIN = NL * T;
    const long long pblk = (long long)blockIdx.x * 256;
    const long long p = pblk + threadIdx.x;
    const bool active = p < a.P;
    const long long pp = active ? p : a.P - 1;
    const long long bimg = pp / a.HW, rem = pp - bimg * a.HW;
    const float x = pixel_x(a, bimg, rem, active);
    const long long lrow = pp - pblk;
    float corr[CIN];
    if constexpr (PRE) {
        LevelWindow<R, BF16> lw[NL];
#pragma unroll
        for (int i = 0; i < NL; ++i) issue_level<R, BF16, true>(lw[i], a, i, x, pblk, lrow);
#pragma unroll
        for (int i = 0; i < NL; ++i)
            finish_level<R, BF16>(lw[i], a, i, pblk, lrow, [&](int t, float v) { corr[i * T + t] = v; });
    } else {
#pragma unroll
        for (int i = 0; i < NL; ++i) {
            LevelWindow<R, BF16> lw;
            issue_level<R, BF16, true>(lw, a, i, x, pblk, lrow);
            finish_level<R, BF16>(lw, a, i, pblk, lrow, [&](int t, float v) { corr[i * T + t] = v; });
        }
    }
    float *op = out + bimg * (long long)cout * a.HW + rem;
    for (int c = 0; c < cout; ++c) {
        const float *wr = wgt + c * CIN;
        float acc = bias ? bias[c] : 0.0f;
#pragma unroll
        for (int k = 0; k < CIN; ++k) acc = fmaf(wr[k], corr[k], acc);
        if (relu) acc = fmaxf(acc, 0.0f);
        if (active) op[(long long)c * a.HW] = acc;
    }
}

template <int R, int M>
static hipError_t launch_chain_m(const LookupArgs &a, hipStream_t s, unsigned lds = 0) {
    const unsigned nblk = (unsigned)((a.P + 255) / 256);
    if (a.levels == 4)
        hipLaunchKernelGGL((lookup_chain_kernel<R, 4, M>), dim3(nblk), dim3(256), lds, s, a);
    else if (a.levels == 3)
        hipLaunchKernelGGL((lookup_chain_kernel<R, 3, M>), dim3(nblk), dim3(256), lds, s, a);
    else
        return hipErrorInvalidValue;
    return hipGetLastError();
}

#ifdef RAFTCORR_DEV
#include "dev/lookup_dev.inc"   // A/B variants and prototypes: libraftcorr_dev.so only
#endif

template <int R>
static hipError_t launch_pair_r(const LookupArgs &a, int bf16, hipStream_t s) {
    const unsigned nblk = (unsigned)((a.P + 255) / 256);
    if (a.rec_nr) {   // RC_LAYOUT_RECORDS (bf16, 4 levels: checked by the C-ABI)
        if (!bf16 || a.levels != 4) return hipErrorNotSupported;
#ifdef RAFTCORR_DEV
        if (const hipError_t e = dev_launch_records<R>(a, s); e != hipErrorNotSupported) return e;
#endif
        if (a.out_dt) return rc_launch_lookup_pair_half(a, R, bf16, s);   // RC_OUT_F16 / RC_OUT_BF16
        // the cooperative whole-record fetch: 118.4 vs 121.5 us per config-3
        // lookup (interleaved, bit-identical; profiles/r06/rec_o)
        if (a.out_cl) hipLaunchKernelGGL((lookup_records_kernel<R, true, 0, true>), dim3(nblk), dim3(256), 0, s, a);
        else hipLaunchKernelGGL((lookup_records_kernel<R, false, 0, true>), dim3(nblk), dim3(256), 0, s, a);
        return hipGetLastError();
    }
    if (a.shk[0]) {   // RC_LAYOUT_DISPARITY (fp32, NCHW output: checked by the C-ABI)
        if (bf16 || a.out_cl || a.out_dt) return hipErrorNotSupported;
        if (a.levels == 4) hipLaunchKernelGGL((lookup_sheared_pair_kernel<R, 4>), dim3(nblk), dim3(256), 0, s, a);
        else if (a.levels == 2) hipLaunchKernelGGL((lookup_sheared_pair_kernel<R, 2>), dim3(nblk), dim3(256), 0, s, a);
        else return hipErrorInvalidValue;
        return hipGetLastError();
    }
#ifdef RAFTCORR_DEV
    if (const hipError_t e = dev_launch_pair<R>(a, bf16, s); e != hipErrorNotSupported) return e;
#endif
    if (a.out_dt) return rc_launch_lookup_pair_half(a, R, bf16, s);       // RC_OUT_F16 / RC_OUT_BF16
    const bool cl = a.out_cl != 0;
    if (a.levels == 4) {
        if (cl) {
            if (bf16) hipLaunchKernelGGL((lookup_pair_kernel<R, 4, 0, true, 1, true>), dim3(nblk), dim3(256), 0, s, a);
            else hipLaunchKernelGGL((lookup_pair_kernel<R, 4, 0, false, 1, true>), dim3(nblk), dim3(256), 0, s, a);
        } else {
            if (bf16) hipLaunchKernelGGL((lookup_pair_kernel<R, 4, 0, true>), dim3(nblk), dim3(256), 0, s, a);
            else hipLaunchKernelGGL((lookup_pair_kernel<R, 4>), dim3(nblk), dim3(256), 0, s, a);
        }
    } else if (a.levels == 2) {
        if (cl) {
            if (bf16) hipLaunchKernelGGL((lookup_pair_kernel<R, 2, 0, true, 1, true>), dim3(nblk), dim3(256), 0, s, a);
            else hipLaunchKernelGGL((lookup_pair_kernel<R, 2, 0, false, 1, true>), dim3(nblk), dim3(256), 0, s, a);
        } else {
            if (bf16) hipLaunchKernelGGL((lookup_pair_kernel<R, 2, 0, true>), dim3(nblk), dim3(256), 0, s, a);
            else hipLaunchKernelGGL((lookup_pair_kernel<R, 2>), dim3(nblk), dim3(256), 0, s, a);
        }
    } else {
        return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

template <int R>
static hipError_t launch_chain_r(const LookupArgs &a, hipStream_t s) {
#ifdef RAFTCORR_DEV
    if (const hipError_t e = dev_launch_chain<R>(a, s); e != hipErrorNotSupported) return e;
#endif
    return launch_chain_m<R, 0>(a, s);
}

template <int R>
static hipError_t launch_conv_r(const LookupArgs &a, int bf16, const float *w, const float *b,
                                int cout, int relu, float *out, hipStream_t s) {
    const unsigned nblk = (unsigned)((a.P + 255) / 256);
#ifdef RAFTCORR_DEV
    if (const hipError_t e = dev_launch_conv<R>(a, bf16, w, b, cout, relu, out, s); e != hipErrorNotSupported)
        return e;
#endif
    if (a.levels == 4) {
        if (bf16) hipLaunchKernelGGL((lookup_conv_kernel<R, 4, true>), dim3(nblk), dim3(256), 0, s, a, w, b, cout, relu, out);
        else hipLaunchKernelGGL((lookup_conv_kernel<R, 4, false>), dim3(nblk), dim3(256), 0, s, a, w, b, cout, relu, out);
    } else if (a.levels == 3) {
        if (bf16) hipLaunchKernelGGL((lookup_conv_kernel<R, 3, true>), dim3(nblk), dim3(256), 0, s, a, w, b, cout, relu, out);
        else hipLaunchKernelGGL((lookup_conv_kernel<R, 3, false>), dim3(nblk), dim3(256), 0, s, a, w, b, cout, relu, out);
    } else if (a.levels == 2) {
        if (bf16) hipLaunchKernelGGL((lookup_conv_kernel<R, 2, true>), dim3(nblk), dim3(256), 0, s, a, w, b, cout, relu, out);
        else hipLaunchKernelGGL((lookup_conv_kernel<R, 2, false>), dim3(nblk), dim3(256), 0, s, a, w, b, cout, relu, out);
    } else {
        return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

template <int R>
static hipError_t launch_r(const LookupArgs &a, int bf16, hipStream_t s) {
    // Default: runtime level loop (low VGPR count, 8 waves/SIMD) + exact-span
    // predicated loads; small problems: every level's loads up front (64-thread
    // blocks) or one wave per level (lookup_levelpar_kernel).  Measured
    // (tools/ablate.py) before choosing.
#ifdef RAFTCORR_DEV
    if (const hipError_t e = dev_launch_level<R>(a, bf16, s); e != hipErrorNotSupported) return e;
#endif
    const bool unroll = a.levels == 3 || a.levels == 4;
    if (a.P < kLevelParP && a.levels <= 4) {
        const unsigned nblk = (unsigned)((a.P + 63) / 64);
        if (bf16) hipLaunchKernelGGL((lookup_levelpar_kernel<R, true>), dim3(nblk), dim3(64 * a.levels), 0, s, a);
        else hipLaunchKernelGGL((lookup_levelpar_kernel<R, false>), dim3(nblk), dim3(64 * a.levels), 0, s, a);
    } else if (a.P < kSmallP && unroll) {
        if (a.levels == 4) {
            if (bf16) launch_k<R, 4, true, true, 64>(a, s);
            else launch_k<R, 4, false, true, 64>(a, s);
        } else {
            if (bf16) launch_k<R, 3, true, true, 64>(a, s);
            else launch_k<R, 3, false, true, 64>(a, s);
        }
    } else {
        if (bf16) launch_k<R, 0, true, true>(a, s);
        else launch_k<R, 0, false, true>(a, s);
    }
    return hipGetLastError();
}

}  // namespace rc

hipError_t rc_launch_lookup(const rc::LookupArgs &a, int radius, int pyr_bf16, hipStream_t s) {
    if (a.P <= 0) return hipSuccess;
    switch (radius) {
        case 1: return rc::launch_r<1>(a, pyr_bf16, s);
        case 2: return rc::launch_r<2>(a, pyr_bf16, s);
        case 3: return rc::launch_r<3>(a, pyr_bf16, s);
        case 4: return rc::launch_r<4>(a, pyr_bf16, s);
        case 5: return rc::launch_r<5>(a, pyr_bf16, s);
        case 6: return rc::launch_r<6>(a, pyr_bf16, s);
        case 7: return rc::launch_r<7>(a, pyr_bf16, s);
        case 8: return rc::launch_r<8>(a, pyr_bf16, s);
        default: return hipErrorInvalidValue;
    }
}

hipError_t rc_launch_lookup_pair(const rc::LookupArgs &a, int radius, int pyr_bf16, hipStream_t s) {
    if (a.P <= 0) return hipSuccess;
    switch (radius) {
        case 1: return rc::launch_pair_r<1>(a, pyr_bf16, s);
        case 2: return rc::launch_pair_r<2>(a, pyr_bf16, s);
        case 3: return rc::launch_pair_r<3>(a, pyr_bf16, s);
        case 4: return rc::launch_pair_r<4>(a, pyr_bf16, s);
        default: return hipErrorInvalidValue;
    }
}

hipError_t rc_launch_lookup_chain(const rc::LookupArgs &a, int radius, hipStream_t s) {
    if (a.P <= 0) return hipSuccess;
    switch (radius) {
        case 1: return rc::launch_chain_r<1>(a, s);
        case 2: return rc::launch_chain_r<2>(a, s);
        case 3: return rc::launch_chain_r<3>(a, s);
        case 4: return rc::launch_chain_r<4>(a, s);
        default: return hipErrorInvalidValue;
    }
}

hipError_t rc_launch_lookup_conv(const rc::LookupArgs &a, int radius, int pyr_bf16, const float *w,
                                 const float *b, int cout, int relu, float *out, hipStream_t s) {
    if (a.P <= 0) return hipSuccess;
    switch (radius) {
        case 1: return rc::launch_conv_r<1>(a, pyr_bf16, w, b, cout, relu, out, s);
        case 2: return rc::launch_conv_r<2>(a, pyr_bf16, w, b, cout, relu, out, s);
        case 3: return rc::launch_conv_r<3>(a, pyr_bf16, w, b, cout, relu, out, s);
        case 4: return rc::launch_conv_r<4>(a, pyr_bf16, w, b, cout, relu, out, s);
        default: return hipErrorInvalidValue;
    }
}
