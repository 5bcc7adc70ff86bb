// The lookup fused with the motion encoder's convc1 (+ ReLU) on the PAIR
// layout, forward and backward (rc_corr_lookup_chain_conv,
// rc_corr_lookup_chain_conv_backward; gfx950).
//
// lookup_conv_kernel (lookup.hip) and lookup_conv_bwd_kernel
// (lookup_conv_bwd.hip) recompute the correlation one window per level, so
// they need every level in memory.  The kernels here obtain the same corr[]
// the way lookup_pair_kernel does -- levels 0 and 2 stored (with their
// RC_SHADOW copies where given), levels 1 and 3 derived in registers from the
// same spans -- so a block that stores the pair layout never has to pool the
// derived levels for the fused path, and a pixel reads ~2.8 instead of ~4.4
// 128-B lines.
//   lookup half: plan_pair_loads / load_pair / span_shift / finish_span of
//     lookup_pair.h, the pair kernel's load schedule (span 2's loads issue
//     between span 0's two levels), with a sink that keeps the channel in a
//     register: corr[] is the pair kernel's output, i.e. the per-level
//     kernels', bit for bit;
//   conv half (forward): lookup_conv_kernel's chain -- bias, then one fmaf
//     per k ascending, then fmaxf -- so the fp32 result is lookup_conv_kernel's
//     bit for bit; rounded once to OT (out_cvt) for RC_OUT_F16 / RC_OUT_BF16,
//     i.e. Tensor.to(dtype) of the fp32 result;
//   backward: conv_bwd_sums (lookup_conv_bwd.h), the per-level backward's code
//     after its recompute, with that kernel's pixel-to-workgroup assignment,
//     followed by the same lookup_conv_bwd_reduce_kernel: the three gradients
//     are the per-level backward's bit for bit.
// Built with -ffp-contract=off like lookup.hip.
#include "lookup_conv_bwd.h"
#include "lookup_pair.h"

namespace rc {

// The pixel's NL*(2R+1) correlation values from its pair spans, in the pair
// kernel's schedule (lookup_pair_kernel): span 0's loads,
// span 2's address math while they fly, level 0's taps, span 2's loads, level
// 1's taps while those fly, then levels 2 and 3.
template <int R, int NL, bool BF16>
__device__ __forceinline__ void pair_corr(const LookupArgs &a, const PairPixel &q, float *corr) {
    static_assert(NL == 2 || NL == 4, "pair lookup: 2 or 4 levels");
    constexpr int NP = NL / 2;
    PairSpan<R, BF16> sp[NP];
    PairLoads<R, BF16> pl[NP];
    pl[0] = plan_pair_loads<R, BF16>(sp[0], a, 0, q.x, q.pblk, q.lrow);
    load_pair<R, BF16>(sp[0], pl[0]);
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (NP > 1) pl[1] = plan_pair_loads<R, BF16>(sp[1], a, 2, q.x, q.pblk, q.lrow);
    auto sink = [&](int ch, float v) { corr[ch] = v; };
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        float s[PairSpan<R, BF16>::NS];
        span_shift<R, BF16>(sp[k], s);
        auto next = [&] {
            if constexpr (NP > 1) {
                if (k == 0) {
                    __builtin_amdgcn_sched_barrier(0);
                    load_pair<R, BF16>(sp[1], pl[1]);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        };
        finish_span<R, false, BF16>(sp[k], s, a, 2 * k, q.x, q.pp, sink, next);
        __builtin_amdgcn_sched_barrier(0);
    }
}

// Output [B][cout][H][W1] of OT (a.out): one store per lane and channel plane,
// coalesced along w1.  Weights and bias are read with wave-uniform addresses
// (scalar loads); cout is a runtime loop.
template <int R, int NL, bool BF16, class OT>
__global__ __launch_bounds__(256) void lookup_pair_conv_kernel(LookupArgs a, const float *__restrict__ wgt,
                                                               const float *__restrict__ bias, int cout,
                                                               int relu) {
    constexpr int CIN = NL * (2 * R + 1);
    const int blk = xcd_remap(blockIdx.x, gridDim.x);
    const PairPixel q = pair_pixel<R, NL>(a, (long long)blk * 256);
    float corr[CIN];
    pair_corr<R, NL, BF16>(a, q, corr);
    const long long bimg = q.pp / a.HW, rem = q.pp - bimg * a.HW;
    OT *op = reinterpret_cast<OT *>(a.out) + bimg * (long long)cout * a.HW + rem;
    for (int c = 0; c < cout; ++c) {
        const float *wr = wgt + c * CIN;
        float acc = bias ? bias[c] : 0.0f;
#pragma unroll
        for (int k = 0; k < CIN; ++k) acc = fmaf(wr[k], corr[k], acc);
        if (relu) acc = fmaxf(acc, 0.0f);
        // out_cvt's opaque copy: without ReLU the last fmaf and the convert
        // would otherwise fold into one v_fma_mixlo_f16 (one rounding, not two)
        if (q.active) op[(long long)c * a.HW] = out_cvt<OT>(acc);
    }
}

// Workgroup b owns pixels [256 b, 256 b + 256) in hardware block order, as in
// lookup_conv_bwd_kernel: its workspace slice and hence the reduce kernel's
// summation order depend on it.
template <int R, int NL, bool BF16>
__global__ __launch_bounds__(256) void lookup_pair_conv_grad_kernel(LookupArgs a, const float *__restrict__ wgt,
                                                                    const float *__restrict__ bias, int cout,
                                                                    int relu, const float *__restrict__ gout,
                                                                    float *__restrict__ gcorr,
                                                                    float *__restrict__ ws) {
    constexpr int CIN = NL * (2 * R + 1);
    __shared__ float s_corr[4 * CIN * kCbwdPitch];
    __shared__ float s_g[4 * kCbwdGTile];
    const PairPixel q = pair_pixel<R, NL>(a, (long long)blockIdx.x * 256);
    float corr[CIN];
    pair_corr<R, NL, BF16>(a, q, corr);
    const long long bimg = q.pp / a.HW, rem = q.pp - bimg * a.HW;
    conv_bwd_sums<CIN>(corr, a, q.active, bimg, rem, s_corr, s_g, wgt, bias, cout, relu, gout, gcorr, ws);
}

template <int R, int NL, class OT>
static void launch_pconv_o(const LookupArgs &a, int bf16, const float *w, const float *b, int cout, int relu,
                           hipStream_t s) {
    const dim3 g((unsigned)((a.P + 255) / 256)), t(256);
    if (bf16) hipLaunchKernelGGL((lookup_pair_conv_kernel<R, NL, true, OT>), g, t, 0, s, a, w, b, cout, relu);
    else hipLaunchKernelGGL((lookup_pair_conv_kernel<R, NL, false, OT>), g, t, 0, s, a, w, b, cout, relu);
}

template <int R, int NL>
static hipError_t launch_pconv_l(const LookupArgs &a, int bf16, const float *w, const float *b, int cout,
                                 int relu, hipStream_t s) {
    if (a.out_dt == 0) launch_pconv_o<R, NL, float>(a, bf16, w, b, cout, relu, s);
    else if (a.out_dt == 1) launch_pconv_o<R, NL, _Float16>(a, bf16, w, b, cout, relu, s);
    else if (a.out_dt == 2) launch_pconv_o<R, NL, __bf16>(a, bf16, w, b, cout, relu, s);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

template <int R>
static hipError_t launch_pconv_r(const LookupArgs &a, int bf16, const float *w, const float *b, int cout,
                                 int relu, hipStream_t s) {
    if (a.levels == 4) return launch_pconv_l<R, 4>(a, bf16, w, b, cout, relu, s);
    if (a.levels == 2) return launch_pconv_l<R, 2>(a, bf16, w, b, cout, relu, s);
    return hipErrorInvalidValue;
}

template <int R, int NL>
static void launch_pgrad_l(const LookupArgs &a, int bf16, const float *w, const float *b, int cout, int relu,
                           const float *gout, float *gcorr, float *ws, hipStream_t s) {
    const dim3 g((unsigned)((a.P + 255) / 256)), t(256);
    if (bf16)
        hipLaunchKernelGGL((lookup_pair_conv_grad_kernel<R, NL, true>), g, t, 0, s, a, w, b, cout, relu, gout,
                           gcorr, ws);
    else
        hipLaunchKernelGGL((lookup_pair_conv_grad_kernel<R, NL, false>), g, t, 0, s, a, w, b, cout, relu, gout,
                           gcorr, ws);
}

template <int R>
static hipError_t launch_pgrad_r(const LookupArgs &a, int bf16, const float *w, const float *b, int cout,
                                 int relu, const float *gout, float *gcorr, float *ws, hipStream_t s) {
    if (a.levels == 4) launch_pgrad_l<R, 4>(a, bf16, w, b, cout, relu, gout, gcorr, ws, s);
    else if (a.levels == 2) launch_pgrad_l<R, 2>(a, bf16, w, b, cout, relu, gout, gcorr, ws, s);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

}  // namespace rc

hipError_t rc_launch_lookup_pair_conv(const rc::LookupArgs &a, int radius, int pyr_bf16, const float *w,
                                      const float *b, int cout, int relu, hipStream_t s) {
    if (a.P <= 0) return hipSuccess;
    if (a.rec_nr || a.shk[0] || a.out_cl) return hipErrorNotSupported;   // rows, NCHW (checked by the C-ABI)
    switch (radius) {
        case 1: return rc::launch_pconv_r<1>(a, pyr_bf16, w, b, cout, relu, s);
        case 2: return rc::launch_pconv_r<2>(a, pyr_bf16, w, b, cout, relu, s);
        case 3: return rc::launch_pconv_r<3>(a, pyr_bf16, w, b, cout, relu, s);
        case 4: return rc::launch_pconv_r<4>(a, pyr_bf16, w, b, cout, relu, s);
        default: return hipErrorInvalidValue;
    }
}

hipError_t rc_launch_lookup_pair_conv_bwd(const rc::LookupArgs &a, int radius, int pyr_bf16, const float *w,
                                          const float *b, int cout, int relu, const float *grad_out,
                                          float *grad_corr, float *grad_weight, float *grad_bias,
                                          float *workspace, hipStream_t s) {
    if (a.P <= 0) return hipSuccess;
    if (a.rec_nr || a.shk[0]) return hipErrorNotSupported;
    const bool sums = grad_weight || grad_bias;
    float *ws = sums ? workspace : nullptr;
    hipError_t e;
    switch (radius) {
        case 1: e = rc::launch_pgrad_r<1>(a, pyr_bf16, w, b, cout, relu, grad_out, grad_corr, ws, s); break;
        case 2: e = rc::launch_pgrad_r<2>(a, pyr_bf16, w, b, cout, relu, grad_out, grad_corr, ws, s); break;
        case 3: e = rc::launch_pgrad_r<3>(a, pyr_bf16, w, b, cout, relu, grad_out, grad_corr, ws, s); break;
        case 4: e = rc::launch_pgrad_r<4>(a, pyr_bf16, w, b, cout, relu, grad_out, grad_corr, ws, s); break;
        default: return hipErrorInvalidValue;
    }
    if (e != hipSuccess || !sums) return e;
    return rc_launch_lookup_conv_bwd_reduce(ws, (int)((a.P + 255) / 256), cout, a.levels * (2 * radius + 1),
                                            grad_weight, grad_bias, s);
}
