// Correlation volume + fused pyramid epilogue for an fp16 pyramid (RC_F16;
// gfx950): the 16-bit MFMA kernels of volume_b16.h instantiated with
// EK = kF16, i.e. v_mfma_f32_16x16x32_f16 (the bf16 instruction's rate) on
// fp16 operands -- fp16 feature maps as they are, or fp32 ones rounded to
// fp16 on load -- and levels stored as fp16.  The LDS-DMA ring, the LDS
// images and the ds_read_b64_tr_b16 fragment reads are the bf16 kernels':
// they move 16-bit payloads.  Semantics mirror the bf16 pyramid (DESIGN.md
// §3.1d): the fp32 accumulator is scaled by 1/sqrt(D) in fp32 and rounded
// once (v_cvt_f16_f32: nearest even, subnormals kept, above 65504 -> +-inf,
// as Tensor.half()) for level 0; every higher level is fp16((x + y) * 0.5f) of
// the level below AS STORED.  Its own translation unit, like lookup_half.hip:
// the instantiations compile beside volume.hip, not after it.
#include "volume_b16.h"

namespace rc {

template <bool IN_F16, bool ALIGNED>
static void launch_f16_pw(const BuildArgs &a, unsigned nwg, hipStream_t s) {
    hipLaunchKernelGGL((build_bf16_kernel<IN_F16, ALIGNED, 0, kF16>), dim3(nwg), dim3(256), 0, s, a, (int)nwg);
}

}  // namespace rc

// fp16 MFMA build; rc_launch_build_bf16mma's choice of kernel (the ring for
// fp16 fmaps inside bf16_ring_shape's rules, else the per-wave kernel).  The
// ring fuses at most kB16MaxFused levels: a.nfused is lowered to what was
// written, and the caller pools the rest.
hipError_t rc_launch_build_f16mma(rc::BuildArgs &a, int in_16, hipStream_t s) {
    const long long nwg = (long long)a.B * a.H * a.tiles_m * a.tiles_n;
    if (nwg <= 0) return hipSuccess;
    if (nwg > 0x7FFFFFFF) return hipErrorInvalidValue;
    if (a.rec || a.pyr_bf16 != rc::kF16) return hipErrorNotSupported;   // records: bf16 only
    const unsigned n = (unsigned)nwg;
    const rc::B16Shape sh = in_16 ? rc::bf16_ring_shape(a) : rc::B16Shape{0, 0, false};
    if (sh.nwn) {
        if (a.nfused > rc::kB16MaxFused) a.nfused = rc::kB16MaxFused;
        rc::launch_bf16_ring<0, rc::kF16>(a, sh, s);
        return hipGetLastError();
    }
    if (in_16) {
        if (a.W1 % 8 == 0 && a.W2 % 8 == 0) rc::launch_f16_pw<true, true>(a, n, s);
        else rc::launch_f16_pw<true, false>(a, n, s);
    } else {
        if (a.W1 % 4 == 0 && a.W2 % 4 == 0) rc::launch_f16_pw<false, true>(a, n, s);
        else rc::launch_f16_pw<false, false>(a, n, s);
    }
    return hipGetLastError();
}
