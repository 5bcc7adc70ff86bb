// Backward of the lookup fused with the motion encoder's convc1 (+ ReLU),
// rc_corr_lookup_conv_backward (gfx950).
//
// Forward (lookup_conv_kernel, lookup.hip; model.py:199, :206), per pixel:
//     pre[c] = bias[c] + sum_k W[c][k] corr[k]     (k ascending, one fmaf each)
//     out[c] = relu ? max(pre[c], 0) : pre[c]
// with corr[k] the lookup at the pixel, k = level*(2r+1) + tap.  Backward, with
// g[c] = grad_out[c] * (relu ? pre[c] > 0 : 1):
//     grad_corr[k]    = sum_c W[c][k] g[c]                  per pixel
//     grad_weight[c][k] = sum_pixels g[c] corr[k]
//     grad_bias[c]    = sum_pixels g[c]
// Nothing is kept from the forward: the lane recomputes its pixel's corr with
// the forward's helpers (issue_level / finish_level, every level's loads
// first) and pre[c] in the forward's order, so the ReLU mask is the forward's
// bit for bit.  grad_corr has the layout of rc_corr_lookup's output, i.e. it
// is the grad_out rc_corr_lookup_backward(_calls) consume.
//
// The sums over pixels: a workgroup owns 256 pixels, one lane each, and output
// channels go 16 at a time.  Per 16 channels every wave stages g[16][64] next
// to its corr[CIN][64] in LDS and multiplies them on v_mfma_f32_16x16x4_f32
// with the pixels as K (A = g, B = corr plus one column of ones, which yields
// the bias sum): 16 K-steps x ceil((CIN+1)/16) column tiles.  The four waves'
// fragments are added in wave order through LDS and written to the
// workgroup's slice of the workspace; lookup_conv_bwd_reduce_kernel then adds
// the slices in a fixed order.  No atomics: results repeat bit for bit.
// LDS rows have a pitch of 68 floats: the 64 lanes of an operand read
// (16 rows x 4 consecutive pixels) hit 64 distinct banks.  56.6 KB per
// workgroup at CIN = 36: two workgroups per CU.
// Everything after the recompute is conv_bwd_sums (lookup_conv_bwd.h), shared
// with the pair-layout backward (lookup_pair_conv.hip), which also launches
// the reduce kernel defined here (rc_launch_lookup_conv_bwd_reduce).
// Built with -ffp-contract=off like lookup.hip (the lookup's op sequence).
#include "common.h"
#include "lookup_conv_bwd.h"   // conv_bwd_sums: everything after the corr recompute
#include "lookup_level.h"

namespace rc {

template <int R, int NL, bool BF16>
__global__ __launch_bounds__(256) void lookup_conv_bwd_kernel(LookupArgs a, const float *__restrict__ wgt,
                                                              const float *__restrict__ bias, int cout,
                                                              int relu, const float *__restrict__ gout,
                                                              float *__restrict__ gcorr,
                                                              float *__restrict__ ws) {
    constexpr int T = 2 * R + 1, CIN = NL * T;
    __shared__ float s_corr[4 * CIN * kCbwdPitch];
    __shared__ float s_g[4 * kCbwdGTile];
    const long long pblk = (long long)blockIdx.x * 256;
    const long long p = pblk + threadIdx.x;
    const bool active = p < a.P;
    const long long pp = active ? p : a.P - 1;
    const long long bimg = pp / a.HW, rem = pp - bimg * a.HW;
    const float x = pixel_x(a, bimg, rem, false);
    const long long lrow = pp - pblk;
    float corr[CIN];
    {
        LevelWindow<R, BF16> lw[NL];
#pragma unroll
        for (int i = 0; i < NL; ++i) issue_level<R, BF16, true>(lw[i], a, i, x, pblk, lrow);
#pragma unroll
        for (int i = 0; i < NL; ++i)
            finish_level<R, BF16>(lw[i], a, i, pblk, lrow, [&](int t, float v) { corr[i * T + t] = v; });
    }
    conv_bwd_sums<CIN>(corr, a, active, bimg, rem, s_corr, s_g, wgt, bias, cout, relu, gout, gcorr, ws);
}

// grad_weight[c][k] / grad_bias[c] = the sum over the nblk workgroup slices
// ws[b][c][cin + 1] (column cin = the bias sum).  A block owns 64 elements;
// each of its four waves adds one contiguous quarter of the slices in order,
// and the quarters are added in order.
__global__ __launch_bounds__(256) void lookup_conv_bwd_reduce_kernel(const float *__restrict__ ws, int nblk,
                                                                     int cout, int cin,
                                                                     float *__restrict__ gw,
                                                                     float *__restrict__ gb) {
    __shared__ float part[4][64];
    const int n = cout * (cin + 1);
    const int l = threadIdx.x & 63, seg = threadIdx.x >> 6;
    const int e = blockIdx.x * 64 + l;
    const int per = (nblk + 3) / 4;
    const int b0 = seg * per, b1 = min(nblk, b0 + per);
    float s = 0.0f;
    if (e < n)
        for (int b = b0; b < b1; ++b) s += ws[(long long)b * n + e];
    part[seg][l] = s;
    __syncthreads();
    if (seg == 0 && e < n) {
        const float tot = ((part[0][l] + part[1][l]) + part[2][l]) + part[3][l];
        const int c = e / (cin + 1), j = e - c * (cin + 1);
        if (j < cin) {
            if (gw) gw[c * cin + j] = tot;
        } else if (gb) {
            gb[c] = tot;
        }
    }
}

template <int R, int NL>
static void launch_cbwd_l(const LookupArgs &a, int bf16, const float *w, const float *b, int cout, int relu,
                          const float *gout, float *gcorr, float *ws, hipStream_t s) {
    const unsigned nblk = (unsigned)((a.P + 255) / 256);
    if (bf16)
        hipLaunchKernelGGL((lookup_conv_bwd_kernel<R, NL, true>), dim3(nblk), dim3(256), 0, s, a, w, b, cout,
                           relu, gout, gcorr, ws);
    else
        hipLaunchKernelGGL((lookup_conv_bwd_kernel<R, NL, false>), dim3(nblk), dim3(256), 0, s, a, w, b, cout,
                           relu, gout, gcorr, ws);
}

template <int R>
static hipError_t launch_cbwd_r(const LookupArgs &a, int bf16, const float *w, const float *b, int cout,
                                int relu, const float *gout, float *gcorr, float *ws, hipStream_t s) {
    if (a.levels == 4) launch_cbwd_l<R, 4>(a, bf16, w, b, cout, relu, gout, gcorr, ws, s);
    else if (a.levels == 3) launch_cbwd_l<R, 3>(a, bf16, w, b, cout, relu, gout, gcorr, ws, s);
    else if (a.levels == 2) launch_cbwd_l<R, 2>(a, bf16, w, b, cout, relu, gout, gcorr, ws, s);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

}  // namespace rc

hipError_t rc_launch_lookup_conv_bwd(const rc::LookupArgs &a, int radius, int pyr_bf16, const float *w,
                                     const float *b, int cout, int relu, const float *grad_out,
                                     float *grad_corr, float *grad_weight, float *grad_bias,
                                     float *workspace, hipStream_t s) {
    if (a.P <= 0) return hipSuccess;
    const bool sums = grad_weight || grad_bias;
    float *ws = sums ? workspace : nullptr;
    hipError_t e;
    switch (radius) {
        case 1: e = rc::launch_cbwd_r<1>(a, pyr_bf16, w, b, cout, relu, grad_out, grad_corr, ws, s); break;
        case 2: e = rc::launch_cbwd_r<2>(a, pyr_bf16, w, b, cout, relu, grad_out, grad_corr, ws, s); break;
        case 3: e = rc::launch_cbwd_r<3>(a, pyr_bf16, w, b, cout, relu, grad_out, grad_corr, ws, s); break;
        case 4: e = rc::launch_cbwd_r<4>(a, pyr_bf16, w, b, cout, relu, grad_out, grad_corr, ws, s); break;
        default: return hipErrorInvalidValue;
    }
    if (e != hipSuccess || !sums) return e;
    return rc_launch_lookup_conv_bwd_reduce(ws, (int)((a.P + 255) / 256), cout, a.levels * (2 * radius + 1),
                                            grad_weight, grad_bias, s);
}

hipError_t rc_launch_lookup_conv_bwd_reduce(const float *ws, int nblk, int cout, int cin, float *grad_weight,
                                            float *grad_bias, hipStream_t s) {
    const int n = cout * (cin + 1);
    hipLaunchKernelGGL(rc::lookup_conv_bwd_reduce_kernel, dim3((unsigned)((n + 63) / 64)), dim3(256), 0, s, ws,
                       nblk, cout, cin, grad_weight, grad_bias);
    return hipGetLastError();
}
