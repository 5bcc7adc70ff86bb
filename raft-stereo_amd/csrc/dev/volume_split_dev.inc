// Dev-library part of volume_split.hip (libraftcorr_dev.so only; included
// inside namespace rc after the product kernel): RAFTCORR_SPLIT_MODE = sums
// of the kMode* ablation flags of epilogue.h (1 no operand loads, 2 no
// epilogue stores, 4 no MFMAs, 512 no MFMA issue, 1024 head piece only,
// 65536 stores into 8 L2-resident rows).  Timing only.
static hipError_t dev_launch_build_split(const BuildArgs &a, long long nwg, int tf1, int tf2, int tiles1,
                                         int tiles2, hipStream_t s) {
    if (a.shk[0] && (dev_knob("RAFTCORR_SPLIT_MODE") || dev_knob("RAFTCORR_SPLIT_RING")))
        return hipErrorNotSupported;   // the knobs select row-layout kernels only (ADVICE r5)
    // RAFTCORR_SPLIT_RING = 103 / 104: the full-width (128) ring with three /
    // four slots on ANY row-layout shape, whatever the product's dispatch
    // (sp_ring3) picks for it: 104 is the kernel every shape ran before the
    // three-slot ring -- the yardstick of the A/B and of the bit-identity
    // test.
    if (!a.shk[0]) {
        const int ring = dev_knob("RAFTCORR_SPLIT_RING");
#define RC_SPLIT_RING_CASE(VAL, M, SLOTS)                                                                          \
    if (ring == VAL) {                                                                                             \
        if (a.nfused <= 3)                                                                                         \
            hipLaunchKernelGGL((build_split_kernel<M, 3, 128, SLOTS>), dim3((unsigned)nwg), dim3(256), 0, s, a,    \
                               (int)nwg, tf1, tf2, tiles1, tiles2);                                                \
        else                                                                                                       \
            hipLaunchKernelGGL((build_split_kernel<M, kSpMaxFused, 128, SLOTS>), dim3((unsigned)nwg), dim3(256),   \
                               0, s, a, (int)nwg, tf1, tf2, tiles1, tiles2);                                       \
        return hipGetLastError();                                                                                  \
    }
        RC_SPLIT_RING_CASE(103, 0, 3)
        RC_SPLIT_RING_CASE(104, 0, 4)
#undef RC_SPLIT_RING_CASE
    }
    switch (dev_knob("RAFTCORR_SPLIT_MODE")) {
    case 1: hipLaunchKernelGGL((build_split_kernel<1, 3>), dim3((unsigned)nwg), dim3(256), 0, s, a, (int)nwg, tf1, tf2, tiles1, tiles2); return hipGetLastError();
    case 2: hipLaunchKernelGGL((build_split_kernel<2, 3>), dim3((unsigned)nwg), dim3(256), 0, s, a, (int)nwg, tf1, tf2, tiles1, tiles2); return hipGetLastError();
    case 3: hipLaunchKernelGGL((build_split_kernel<3, 3>), dim3((unsigned)nwg), dim3(256), 0, s, a, (int)nwg, tf1, tf2, tiles1, tiles2); return hipGetLastError();
    case 4: hipLaunchKernelGGL((build_split_kernel<4, 3>), dim3((unsigned)nwg), dim3(256), 0, s, a, (int)nwg, tf1, tf2, tiles1, tiles2); return hipGetLastError();
    case 5: hipLaunchKernelGGL((build_split_kernel<5, 3>), dim3((unsigned)nwg), dim3(256), 0, s, a, (int)nwg, tf1, tf2, tiles1, tiles2); return hipGetLastError();
    case 65541: hipLaunchKernelGGL((build_split_kernel<65541, 3>), dim3((unsigned)nwg), dim3(256), 0, s, a, (int)nwg, tf1, tf2, tiles1, tiles2); return hipGetLastError();
    case 6: hipLaunchKernelGGL((build_split_kernel<6, 3>), dim3((unsigned)nwg), dim3(256), 0, s, a, (int)nwg, tf1, tf2, tiles1, tiles2); return hipGetLastError();
    case 7: hipLaunchKernelGGL((build_split_kernel<7, 3>), dim3((unsigned)nwg), dim3(256), 0, s, a, (int)nwg, tf1, tf2, tiles1, tiles2); return hipGetLastError();
    case 512: hipLaunchKernelGGL((build_split_kernel<512, 3>), dim3((unsigned)nwg), dim3(256), 0, s, a, (int)nwg, tf1, tf2, tiles1, tiles2); return hipGetLastError();
    case 1024: hipLaunchKernelGGL((build_split_kernel<1024, 3>), dim3((unsigned)nwg), dim3(256), 0, s, a, (int)nwg, tf1, tf2, tiles1, tiles2); return hipGetLastError();
    case 1027: hipLaunchKernelGGL((build_split_kernel<1027, 3>), dim3((unsigned)nwg), dim3(256), 0, s, a, (int)nwg, tf1, tf2, tiles1, tiles2); return hipGetLastError();
    case 515: hipLaunchKernelGGL((build_split_kernel<515, 3>), dim3((unsigned)nwg), dim3(256), 0, s, a, (int)nwg, tf1, tf2, tiles1, tiles2); return hipGetLastError();
    case 65536: hipLaunchKernelGGL((build_split_kernel<65536, 3>), dim3((unsigned)nwg), dim3(256), 0, s, a, (int)nwg, tf1, tf2, tiles1, tiles2); return hipGetLastError();
        default: return hipErrorNotSupported;
    }
}
