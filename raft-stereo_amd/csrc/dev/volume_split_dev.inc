// Dev-library part of volume_split.hip (libraftcorr_dev.so only; included
// inside namespace rc after the product kernel): RAFTCORR_SPLIT_MODE = sums
// of the kMode* ablation flags of epilogue.h (1 no operand loads, 2 no
// epilogue stores, 4 no MFMAs, 512 no MFMA issue, 1024 head piece only, 8192
// packed residuals, 65536 stores into 8 L2-resident rows, 131072 direct
// stores, 262144 / 524288 fast / generic epilogue, 1048576 pair epilogue,
// 268435456 phased K step (all splits, then all MFMAs at s_setprio 3; +3 =
// compute only), 536870912 each fragment's MFMAs at s_setprio 3; +5 = five
// fused levels).  Timing only where the flag says so.
static hipError_t dev_launch_build_split(const BuildArgs &a, long long nwg, int tf1, int tf2, int tiles1,
                                         int tiles2, hipStream_t s) {
    // RAFTCORR_SPLIT_RING (tiles of at most 5 fragments, 3 fused levels): 86
    // the narrow ring, rows 80 wide, 6 slots (two K steps in flight); 84 the
    // narrow rows with 4 slots (41 KB: three workgroups per CU)
    // 85 / 87: the same two kernels on ANY shape, its rows cut into balanced
    // tiles of at most 5 fragments (W = 240: 3 x 3 tiles of 80 instead of
    // 2 x 2 of 128 / 112) -- the third workgroup per CU for wide rows
    if (a.shk[0] && (dev_knob("RAFTCORR_SPLIT_MODE") || dev_knob("RAFTCORR_SPLIT_RING")))
        return hipErrorNotSupported;   // the knobs select row-layout kernels only (ADVICE r5)
    if (!a.shk[0] && a.nfused <= 3 && (dev_knob("RAFTCORR_SPLIT_RING") >= 100 && dev_knob("RAFTCORR_SPLIT_RING") <= 102)) {
        // split once per workgroup into LDS planes (build_split_planes_kernel)
        return rc_launch_build_planes(const_cast<BuildArgs &>(a), s);
    }
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
    if (!a.shk[0] && a.nfused <= 3) {
        const int ring = dev_knob("RAFTCORR_SPLIT_RING");
        if (ring == 85 || ring == 87) {
            auto frags5 = [](int W) {
                const int nf = (W + 15) / 16, nt = (nf + 4) / 5;
                return (nf + nt - 1) / nt;
            };
            const int f1 = frags5(a.W1), f2 = frags5(a.W2);
            const int t1 = ((a.W1 + 15) / 16 + f1 - 1) / f1, t2 = ((a.W2 + 15) / 16 + f2 - 1) / f2;
            const long long n = (long long)a.B * a.H * t1 * t2;
            if (n > 0x7FFFFFFF) return hipErrorInvalidValue;
            if (ring == 85)
                hipLaunchKernelGGL((build_split_kernel<0, 3, 80, 4>), dim3((unsigned)n), dim3(256), 0, s, a, (int)n, f1, f2, t1, t2);
            else
                hipLaunchKernelGGL((build_split_kernel<0, 3, 80, 6>), dim3((unsigned)n), dim3(256), 0, s, a, (int)n, f1, f2, t1, t2);
            return hipGetLastError();
        }
    }
    if (!a.shk[0] && a.nfused <= 3 && tf1 <= 5 && tf2 <= 5) {
        const int ring = dev_knob("RAFTCORR_SPLIT_RING");
        if (ring == 86) {
            hipLaunchKernelGGL((build_split_kernel<0, 3, 80, 6>), dim3((unsigned)nwg), dim3(256), 0, s, a, (int)nwg, tf1, tf2, tiles1, tiles2);
            return hipGetLastError();
        }
        if (ring == 84) {
            hipLaunchKernelGGL((build_split_kernel<0, 3, 80, 4>), dim3((unsigned)nwg), dim3(256), 0, s, a, (int)nwg, tf1, tf2, tiles1, tiles2);
            return hipGetLastError();
        }
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
    case 8192: hipLaunchKernelGGL((build_split_kernel<8192, 3>), dim3((unsigned)nwg), dim3(256), 0, s, a, (int)nwg, tf1, tf2, tiles1, tiles2); return hipGetLastError();
    case 1048576: hipLaunchKernelGGL((build_split_kernel<1048576, 3>), dim3((unsigned)nwg), dim3(256), 0, s, a, (int)nwg, tf1, tf2, tiles1, tiles2); return hipGetLastError();
    case 524288: hipLaunchKernelGGL((build_split_kernel<524288, 3>), dim3((unsigned)nwg), dim3(256), 0, s, a, (int)nwg, tf1, tf2, tiles1, tiles2); return hipGetLastError();
    case 524293: hipLaunchKernelGGL((build_split_kernel<524288, kSpMaxFused>), dim3((unsigned)nwg), dim3(256), 0, s, a, (int)nwg, tf1, tf2, tiles1, tiles2); return hipGetLastError();
    case 262144: hipLaunchKernelGGL((build_split_kernel<262144, 3>), dim3((unsigned)nwg), dim3(256), 0, s, a, (int)nwg, tf1, tf2, tiles1, tiles2); return hipGetLastError();
    case 262149: hipLaunchKernelGGL((build_split_kernel<262149, 3>), dim3((unsigned)nwg), dim3(256), 0, s, a, (int)nwg, tf1, tf2, tiles1, tiles2); return hipGetLastError();
    case 131072: hipLaunchKernelGGL((build_split_kernel<131072, 3>), dim3((unsigned)nwg), dim3(256), 0, s, a, (int)nwg, tf1, tf2, tiles1, tiles2); return hipGetLastError();
    case 131077: hipLaunchKernelGGL((build_split_kernel<131072, kSpMaxFused>), dim3((unsigned)nwg), dim3(256), 0, s, a, (int)nwg, tf1, tf2, tiles1, tiles2); return hipGetLastError();
    case 65536: hipLaunchKernelGGL((build_split_kernel<65536, 3>), dim3((unsigned)nwg), dim3(256), 0, s, a, (int)nwg, tf1, tf2, tiles1, tiles2); return hipGetLastError();
    case 268435456: hipLaunchKernelGGL((build_split_kernel<kModePhasePrio | kModeFastEpi, 3>), dim3((unsigned)nwg), dim3(256), 0, s, a, (int)nwg, tf1, tf2, tiles1, tiles2); return hipGetLastError();
    case 536870912: hipLaunchKernelGGL((build_split_kernel<kModeMfmaPrio | kModeFastEpi, 3>), dim3((unsigned)nwg), dim3(256), 0, s, a, (int)nwg, tf1, tf2, tiles1, tiles2); return hipGetLastError();
    case 268435459: hipLaunchKernelGGL((build_split_kernel<kModePhasePrio | 3, 3>), dim3((unsigned)nwg), dim3(256), 0, s, a, (int)nwg, tf1, tf2, tiles1, tiles2); return hipGetLastError();
        default: return hipErrorNotSupported;
    }
}
