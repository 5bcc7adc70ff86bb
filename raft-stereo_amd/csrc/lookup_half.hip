// The pair and records lookups with an fp16 / bf16 output (RC_OUT_F16 /
// RC_OUT_BF16, ABI v13; gfx950): the kernels of lookup_pair.h instantiated
// with a 2-byte output element, for the consumer that would cast the fp32
// output anyway (the update block under autocast).  Loads, spans and tap math
// are the fp32-output kernels'; the final fp32 value is rounded once, in the
// sink (out_cvt), so the result is Tensor.to(dtype) of the fp32 output bit
// for bit while the output write -- the largest term of the lookup's traffic
// -- halves and the consumer's cast kernel goes away.
// Its own translation unit: the instantiations (radius 1..4 x 2 / 4 levels x
// pyramid dtype x NCHW / channels-last x 2 output types, and the records
// kernel) compile beside lookup.hip, not after it.  Built with
// -ffp-contract=off like lookup.hip.
#include "lookup_pair.h"

namespace rc {

template <int R, class OT>
static hipError_t launch_pair_half(const LookupArgs &a, int bf16, hipStream_t s) {
    const unsigned nblk = (unsigned)((a.P + 255) / 256);
    const dim3 g(nblk), b(256);
    if (a.rec_nr) {   // RC_LAYOUT_RECORDS (bf16, 4 levels: checked by the C-ABI and rc_launch_lookup_pair)
        if (a.out_cl) hipLaunchKernelGGL((lookup_records_kernel<R, true, 0, true, 1, OT>), g, b, 0, s, a);
        else hipLaunchKernelGGL((lookup_records_kernel<R, false, 0, true, 1, OT>), g, b, 0, s, a);
        return hipGetLastError();
    }
    if (a.shk[0]) return hipErrorNotSupported;   // RC_LAYOUT_DISPARITY writes fp32 only
    const bool cl = a.out_cl != 0;
    if (a.levels == 4) {
        if (cl) {
            if (bf16) hipLaunchKernelGGL((lookup_pair_kernel<R, 4, 0, true, 1, true, OT>), g, b, 0, s, a);
            else hipLaunchKernelGGL((lookup_pair_kernel<R, 4, 0, false, 1, true, OT>), g, b, 0, s, a);
        } else {
            if (bf16) hipLaunchKernelGGL((lookup_pair_kernel<R, 4, 0, true, 1, false, OT>), g, b, 0, s, a);
            else hipLaunchKernelGGL((lookup_pair_kernel<R, 4, 0, false, 1, false, OT>), g, b, 0, s, a);
        }
    } else if (a.levels == 2) {
        if (cl) {
            if (bf16) hipLaunchKernelGGL((lookup_pair_kernel<R, 2, 0, true, 1, true, OT>), g, b, 0, s, a);
            else hipLaunchKernelGGL((lookup_pair_kernel<R, 2, 0, false, 1, true, OT>), g, b, 0, s, a);
        } else {
            if (bf16) hipLaunchKernelGGL((lookup_pair_kernel<R, 2, 0, true, 1, false, OT>), g, b, 0, s, a);
            else hipLaunchKernelGGL((lookup_pair_kernel<R, 2, 0, false, 1, false, OT>), g, b, 0, s, a);
        }
    } else {
        return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

template <int R>
static hipError_t launch_pair_half_r(const LookupArgs &a, int bf16, hipStream_t s) {
    if (a.out_dt == 1) return launch_pair_half<R, _Float16>(a, bf16, s);
    if (a.out_dt == 2) return launch_pair_half<R, __bf16>(a, bf16, s);
    return hipErrorInvalidValue;
}

}  // namespace rc

hipError_t rc_launch_lookup_pair_half(const rc::LookupArgs &a, int radius, int pyr_bf16, hipStream_t s) {
    if (a.P <= 0) return hipSuccess;
    if (a.rec_nr && (!pyr_bf16 || a.levels != 4)) return hipErrorNotSupported;
    switch (radius) {
        case 1: return rc::launch_pair_half_r<1>(a, pyr_bf16, s);
        case 2: return rc::launch_pair_half_r<2>(a, pyr_bf16, s);
        case 3: return rc::launch_pair_half_r<3>(a, pyr_bf16, s);
        case 4: return rc::launch_pair_half_r<4>(a, pyr_bf16, s);
        default: return hipErrorInvalidValue;
    }
}
