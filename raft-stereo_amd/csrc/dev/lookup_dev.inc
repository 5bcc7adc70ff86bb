// Dev-library part of lookup.hip (built only into libraftcorr_dev.so with
// -DRAFTCORR_DEV; included inside namespace rc after every product kernel).
// The A/B launch variants, chosen per call by environment knobs, and the
// disparity-major probe entry.  Each dev_launch_* returns hipErrorNotSupported
// when no knob asks for a variant: the product launcher then runs.

// RAFTCORR_LOOKUP_VARIANT on the pair layout (4 levels, r = 4): 201 no output
// stores, 202 no fallback path, 205 hardware block order, 207 non-temporal
// output stores, 208 / 209 at least 5 / 6 waves per SIMD, 211 the
// channels-last store path into an NCHW buffer.
template <int R>
static hipError_t dev_launch_pair(const LookupArgs &a, int bf16, hipStream_t s) {
    if constexpr (R != 4) {
        return hipErrorNotSupported;
    } else {
        const int v = dev_knob("RAFTCORR_LOOKUP_VARIANT");
        if (a.shk[0] || a.out_dt) return hipErrorNotSupported;   // fp16 / bf16 output: the product kernel
        if (a.levels != 4 || v < 201 || v > 211) return hipErrorNotSupported;
        const unsigned nblk = (unsigned)((a.P + 255) / 256);
#define RC_PAIR(...)                                                                              \
    do {                                                                                          \
        if (bf16) hipLaunchKernelGGL((lookup_pair_kernel<R, 4, __VA_ARGS__, true>), dim3(nblk), dim3(256), 0, s, a); \
        else hipLaunchKernelGGL((lookup_pair_kernel<R, 4, __VA_ARGS__, false>), dim3(nblk), dim3(256), 0, s, a); \
    } while (0)
        switch (v) {
            case 201: RC_PAIR(1); break;
            case 202: RC_PAIR(2); break;
            case 205: RC_PAIR(5); break;
            case 207: RC_PAIR(7); break;
            case 211: RC_PAIR(9); break;
            case 208:
                if (bf16) hipLaunchKernelGGL((lookup_pair_kernel<R, 4, 0, true, 5>), dim3(nblk), dim3(256), 0, s, a);
                else hipLaunchKernelGGL((lookup_pair_kernel<R, 4, 0, false, 5>), dim3(nblk), dim3(256), 0, s, a);
                break;
            case 209:
                if (bf16) hipLaunchKernelGGL((lookup_pair_kernel<R, 4, 0, true, 6>), dim3(nblk), dim3(256), 0, s, a);
                else hipLaunchKernelGGL((lookup_pair_kernel<R, 4, 0, false, 6>), dim3(nblk), dim3(256), 0, s, a);
                break;
            default: return hipErrorNotSupported;
        }
#undef RC_PAIR
        return hipGetLastError();
    }
}

// RAFTCORR_LOOKUP_VARIANT on the level-1 chain (r = 4): 101-104 the chain
// kernel's ablation modes M = 1..4, 105 non-temporal output stores.
template <int R>
static hipError_t dev_launch_chain(const LookupArgs &a, hipStream_t s) {
    if constexpr (R != 4) {
        return hipErrorNotSupported;
    } else {
        switch (dev_knob("RAFTCORR_LOOKUP_VARIANT")) {
            case 101: return launch_chain_m<R, 1>(a, s);
            case 102: return launch_chain_m<R, 2>(a, s);
            case 103: return launch_chain_m<R, 3>(a, s);
            case 104: return launch_chain_m<R, 4>(a, s);
            case 105: return launch_chain_m<R, 5>(a, s);
            default: return hipErrorNotSupported;
        }
    }
}

// RAFTCORR_CONV_VARIANT=1: the fused convc1 lookup one level at a time.
template <int R>
static hipError_t dev_launch_conv(const LookupArgs &a, int bf16, const float *w, const float *b, int cout,
                                  int relu, float *out, hipStream_t s) {
    if (dev_knob("RAFTCORR_CONV_VARIANT") != 1 || a.levels != 4 || bf16) return hipErrorNotSupported;
    const unsigned nblk = (unsigned)((a.P + 255) / 256);
    hipLaunchKernelGGL((lookup_conv_kernel<R, 4, false, false>), dim3(nblk), dim3(256), 0, s, a, w, b, cout, relu, out);
    return hipGetLastError();
}

// (The record-layout prototype of round 5 is the product's
// lookup_records_kernel since round 6: RC_LAYOUT_RECORDS.)
// RAFTCORR_REC_LOOKUP on the record lookup (timing only, wrong output):
// 1 no output stores, 2 no record loads, 3 record loads only (per-lane
// chunk loads, the pre-COOP kernel); 4 the whole records fetched
// cooperatively into LDS (COOP: the product since r06o), 5 / 6 COOP without
// output stores / loads only, 7 / 8 COOP / per-lane loads capped at 4 waves
// per SIMD (128 VGPRs: 5 / 3 spilled), 9 per-lane loads (the pre-COOP product).
template <int R>
static hipError_t dev_launch_records(const LookupArgs &a, hipStream_t s) {
    const int v = dev_knob("RAFTCORR_REC_LOOKUP");
    if (v < 1 || v > 9 || !a.out_cl || a.out_dt) return hipErrorNotSupported;   // fp16 / bf16 output: the product kernel
    const unsigned nblk = (unsigned)((a.P + 255) / 256);
    if (v == 1) hipLaunchKernelGGL((lookup_records_kernel<R, true, 1>), dim3(nblk), dim3(256), 0, s, a);
    else if (v == 2) hipLaunchKernelGGL((lookup_records_kernel<R, true, 2>), dim3(nblk), dim3(256), 0, s, a);
    else if (v == 3) hipLaunchKernelGGL((lookup_records_kernel<R, true, 3>), dim3(nblk), dim3(256), 0, s, a);
    else if (v == 4) hipLaunchKernelGGL((lookup_records_kernel<R, true, 0, true>), dim3(nblk), dim3(256), 0, s, a);
    else if (v == 5) hipLaunchKernelGGL((lookup_records_kernel<R, true, 1, true>), dim3(nblk), dim3(256), 0, s, a);
    else if (v == 6) hipLaunchKernelGGL((lookup_records_kernel<R, true, 3, true>), dim3(nblk), dim3(256), 0, s, a);
    else if (v == 7) hipLaunchKernelGGL((lookup_records_kernel<R, true, 0, true, 4>), dim3(nblk), dim3(256), 0, s, a);
    else if (v == 8) hipLaunchKernelGGL((lookup_records_kernel<R, true, 0, false, 4>), dim3(nblk), dim3(256), 0, s, a);
    else hipLaunchKernelGGL((lookup_records_kernel<R, true, 0, false>), dim3(nblk), dim3(256), 0, s, a);
    return hipGetLastError();
}

// RAFTCORR_LOOKUP_VARIANT on the per-level lookup: 1 full windows (no exact-
// span predication), 3 levels unrolled, 4 the same capped at 4 waves/SIMD,
// 6 the level-parallel kernel with blocks in launch order (no XCD placement).
template <int R>
static hipError_t dev_launch_level(const LookupArgs &a, int bf16, hipStream_t s) {
    const int v = dev_knob("RAFTCORR_LOOKUP_VARIANT");
    if (v == 6 && a.P < kLevelParP && a.levels <= 4) {
        const unsigned nblk = (unsigned)((a.P + 63) / 64);
        if (bf16) hipLaunchKernelGGL((lookup_levelpar_kernel<R, true, false>), dim3(nblk), dim3(64 * a.levels), 0, s, a);
        else hipLaunchKernelGGL((lookup_levelpar_kernel<R, false, false>), dim3(nblk), dim3(64 * a.levels), 0, s, a);
    } else if (v == 1) {
        if (bf16) launch_k<R, 0, true, false>(a, s);
        else launch_k<R, 0, false, false>(a, s);
    } else if (v == 4 && a.levels == 4) {
        if (bf16) launch_k<R, 4, true, true, 256, 4>(a, s);
        else launch_k<R, 4, false, true, 256, 4>(a, s);
    } else if (v == 3 && a.levels == 4) {
        if (bf16) launch_k<R, 4, true, true>(a, s);
        else launch_k<R, 4, false, true>(a, s);
    } else {
        return hipErrorNotSupported;
    }
    return hipGetLastError();
}

}  // namespace rc

// Dev-only entry (tools/shear_probe.py): the disparity-major pair lookup
// (fp32, 4 levels, r = 4) over levels 0 and 2 laid out by the probe itself
// as S_i[b,h][k][w1] (K0 / K2 rows of ldw floats per image row) -- the
// product kernel of RC_LAYOUT_DISPARITY.
extern "C" int rc_dev_lookup_sheared_pair(const void *lvl0, const void *lvl2, long K0, long K2, long ldw,
                                          const int *widths, const float *coords_x, long cbs, int B, int H,
                                          int W1, float *out, void *stream) {
    rc::LookupArgs a{};
    for (int i = 0; i < 4; ++i) a.W[i] = widths[i];
    a.lvl[0] = lvl0;
    a.lvl[2] = lvl2;
    a.ld[0] = a.ld[2] = ldw;
    a.shk[0] = K0;
    a.shk[2] = K2;
    a.coords = coords_x;
    a.cbs = cbs;
    a.out = out;
    a.P = (long long)B * H * W1;
    a.HW = H * W1;
    a.W1 = W1;
    a.levels = 4;
    if (a.P <= 0) return 0;
    const unsigned nblk = (unsigned)((a.P + 255) / 256);
    hipLaunchKernelGGL((rc::lookup_sheared_pair_kernel<4, 4>), dim3(nblk), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream), a);
    return hipGetLastError() == hipSuccess ? 0 : 3;
}


namespace rc {
