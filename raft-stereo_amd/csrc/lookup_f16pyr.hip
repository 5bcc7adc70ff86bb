// The lookups over an fp16 pyramid (RC_F16; gfx950): the per-level lookup
// (issue_level / finish_level, lookup_level.h) and the pair lookup
// (lookup_pair_body, lookup_pair.h) instantiated with the element kind kF16.  Address math,
// load schedule, spans and tap math are the bf16 kernels':
// a level element is 2 bytes, eight per 16-B chunk.  Only the three decode
// sites differ -- a stored element widens with v_cvt_f32_f16 instead of a
// shift, and the derived odd levels (1 and 3 of the pair layout) are rounded
// to fp16 as rc_corr_build / rc_corr_pool would have stored them -- so the
// lazy pair layout equals the materialised pyramid bit for bit.  The output
// side is untouched: fp32, or fp16 / bf16 rounded once in the sink (out_cvt
// and its barrier against v_fma_mixlo_f16).
// The kernels carry names of their own (the bf16 / fp32 kernels keep their
// template lists and instance counts), and this is a translation unit of its
// own, like lookup_half.hip, so lookup.hip's compile time does not grow.
// Built with -ffp-contract=off like lookup.hip.
#include "lookup_pair.h"

namespace rc {

// lookup_kernel<R, 0, ..> (lookup.hip) over fp16 levels: one pixel per lane,
// a runtime loop over the levels (any count), exact-span predicated loads
template <int R>
__global__ __launch_bounds__(256) void lookup_f16pyr_level_kernel(LookupArgs a) {
    constexpr int T = 2 * R + 1;
    const long long pblk = (long long)blockIdx.x * 256;
    const long long p = pblk + threadIdx.x;
    const bool active = p < a.P;
    const long long pp = active ? p : a.P - 1;
    const long long bimg = pp / a.HW, rem = pp - bimg * a.HW;
    const float x = pixel_x(a, bimg, rem, active);
    float *outp = a.out + bimg * (long long)(a.levels * T) * a.HW + rem;
    const long long lrow = pp - pblk;
    for (int i = 0; i < a.levels; ++i) {
        LevelWindow<R, kF16> lw;
        issue_level<R, kF16, true>(lw, a, i, x, pblk, lrow);
        finish_level<R, kF16>(lw, a, i, pblk, lrow, [&](int t, float v) {
            if (active) outp[(long long)(i * T + t) * a.HW] = v;
        });
    }
}

template <int R, int NL, bool CL, class OT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1))) void lookup_f16pyr_pair_kernel(LookupArgs a) {
    lookup_pair_body<R, NL, 0, kF16, CL, OT>(a);
}

template <int R, class OT>
static hipError_t launch_f16pyr_pair(const LookupArgs &a, hipStream_t s) {
    const dim3 g((unsigned)((a.P + 255) / 256)), b(256);
    const bool cl = a.out_cl != 0;
    if (a.levels == 4) {
        if (cl) hipLaunchKernelGGL((lookup_f16pyr_pair_kernel<R, 4, true, OT>), g, b, 0, s, a);
        else hipLaunchKernelGGL((lookup_f16pyr_pair_kernel<R, 4, false, OT>), g, b, 0, s, a);
    } else if (a.levels == 2) {
        if (cl) hipLaunchKernelGGL((lookup_f16pyr_pair_kernel<R, 2, true, OT>), g, b, 0, s, a);
        else hipLaunchKernelGGL((lookup_f16pyr_pair_kernel<R, 2, false, OT>), g, b, 0, s, a);
    } else {
        return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

template <int R>
static hipError_t launch_f16pyr_pair_r(const LookupArgs &a, hipStream_t s) {
    if (a.rec_nr || a.shk[0]) return hipErrorNotSupported;   // records / disparity-major: no fp16 pyramid
    if (a.out_dt == 0) return launch_f16pyr_pair<R, float>(a, s);
    if (a.out_dt == 1) return launch_f16pyr_pair<R, _Float16>(a, s);
    if (a.out_dt == 2) return launch_f16pyr_pair<R, __bf16>(a, s);
    return hipErrorInvalidValue;
}

template <int R>
static hipError_t launch_f16pyr_level(const LookupArgs &a, hipStream_t s) {
    hipLaunchKernelGGL((lookup_f16pyr_level_kernel<R>), dim3((unsigned)((a.P + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace rc

hipError_t rc_launch_lookup_f16pyr(const rc::LookupArgs &a, int radius, hipStream_t s) {
    if (a.P <= 0) return hipSuccess;
    switch (radius) {
        case 1: return rc::launch_f16pyr_level<1>(a, s);
        case 2: return rc::launch_f16pyr_level<2>(a, s);
        case 3: return rc::launch_f16pyr_level<3>(a, s);
        case 4: return rc::launch_f16pyr_level<4>(a, s);
        case 5: return rc::launch_f16pyr_level<5>(a, s);
        case 6: return rc::launch_f16pyr_level<6>(a, s);
        case 7: return rc::launch_f16pyr_level<7>(a, s);
        case 8: return rc::launch_f16pyr_level<8>(a, s);
        default: return hipErrorInvalidValue;
    }
}

hipError_t rc_launch_lookup_pair_f16pyr(const rc::LookupArgs &a, int radius, hipStream_t s) {
    if (a.P <= 0) return hipSuccess;
    switch (radius) {
        case 1: return rc::launch_f16pyr_pair_r<1>(a, s);
        case 2: return rc::launch_f16pyr_pair_r<2>(a, s);
        case 3: return rc::launch_f16pyr_pair_r<3>(a, s);
        case 4: return rc::launch_f16pyr_pair_r<4>(a, s);
        default: return hipErrorInvalidValue;
    }
}
