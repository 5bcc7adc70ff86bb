// Dev-library part of volume.hip (libraftcorr_dev.so only; included inside
// namespace rc after the product kernels).  RAFTCORR_BUILD_MODE selects
// ablation modes; every dev_launch_* returns hipErrorNotSupported (or false)
// when the knob asks for none.

// per-wave bf16 kernel: 1 no operand loads, 2 no stores, 3 neither
template <bool IN_BF16, bool ALIGNED>
static bool dev_launch_bf16_pw(const BuildArgs &a, unsigned nwg, hipStream_t s) {
    switch (dev_knob("RAFTCORR_BUILD_MODE")) {
        case 1: hipLaunchKernelGGL((build_bf16_kernel<IN_BF16, ALIGNED, 1>), dim3(nwg), dim3(256), 0, s, a, (int)nwg); return true;
        case 2: hipLaunchKernelGGL((build_bf16_kernel<IN_BF16, ALIGNED, 2>), dim3(nwg), dim3(256), 0, s, a, (int)nwg); return true;
        case 3: hipLaunchKernelGGL((build_bf16_kernel<IN_BF16, ALIGNED, 3>), dim3(nwg), dim3(256), 0, s, a, (int)nwg); return true;
        default: return false;
    }
}

// bf16 build: 32 the per-wave kernel instead of the ring (``sh`` cleared,
// the product launcher continues); ring ablations (timing only): 40 no
// stores, 41 no DMA, 44 no fragment reads / MFMA, 45 neither, 42 / 43 MFMA
// without fragment reads (and no DMA), 46 no DMA with stores, 47 no DMA no
// MFMA with stores, 54 47 into L2-resident rows, 55 the product into
// L2-resident rows.
static hipError_t dev_launch_bf16mma(BuildArgs &a, B16Shape &sh, hipStream_t s) {
    const int mode = dev_knob("RAFTCORR_BUILD_MODE");
    if (mode == 32) sh = B16Shape{0, 0, false};
    if (!sh.nwn || mode < 40 || mode > 55 || (mode >= 49 && mode <= 53)) return hipErrorNotSupported;
    if (a.nfused > kB16MaxFused) a.nfused = kB16MaxFused;
    switch (mode) {
        case 40: launch_bf16_ring<2>(a, sh, s); break;
        case 41: launch_bf16_ring<3>(a, sh, s); break;
        case 44: launch_bf16_ring<6>(a, sh, s); break;
        case 45: launch_bf16_ring<7>(a, sh, s); break;
        case 42: launch_bf16_ring<18>(a, sh, s); break;
        case 43: launch_bf16_ring<19>(a, sh, s); break;
        case 46: launch_bf16_ring<1>(a, sh, s); break;
        case 47: launch_bf16_ring<5>(a, sh, s); break;
        case 54: launch_bf16_ring<kModeL2Stores | 5>(a, sh, s); break;
        case 55: launch_bf16_ring<kModeL2Stores>(a, sh, s); break;
        default: launch_bf16_ring<10>(a, sh, s); break;
    }
    return hipGetLastError();
}

// record build (RC_LAYOUT_RECORDS), RAFTCORR_REC_MODE (timing only, wrong
// records except 0): 1 records gathered but not stored, 2 stored into 8
// L2-resident image rows, 3 no gather (piece images only), 4 no piece images
// and no gather (the K loop, the LDS footprint and the held registers only)
static hipError_t dev_launch_records(const BuildArgs &a, int nwn, hipStream_t s) {
    const int mode = dev_knob("RAFTCORR_REC_MODE");
    if (mode < 1 || mode > 4 || nwn != 5) return hipErrorNotSupported;
    constexpr int R = kModeRecords;
    switch (mode) {
        case 1: launch_bf16_ring_n<5, 4, 4, R | kModeRecNoStore, true>(a, s); break;
        case 2: launch_bf16_ring_n<5, 4, 4, R | kModeL2Stores, true>(a, s); break;
        case 3: launch_bf16_ring_n<5, 4, 4, R | kModeRecNoEmit, true>(a, s); break;
        default: launch_bf16_ring_n<5, 4, 4, R | kModeNoStores, true>(a, s); break;
    }
    return hipGetLastError();
}

// exact fp32 build: 2 ring without epilogue stores, 4 / 5 a 4- / 5-slot
// ring; 128 + flags the direct-load kernel (1 no operand loads, 2 no stores)
static hipError_t dev_launch_f32(const BuildArgs &a, unsigned n, hipStream_t s) {
    switch (dev_knob("RAFTCORR_BUILD_MODE")) {
        case 2: launch_ring<2>(a, s); break;
        case 4: launch_ring<0, 4>(a, s); break;
        case 5: launch_ring<0, 5>(a, s); break;
        case 128: launch<true, 2, 0>(a, n, s); break;
        case 129: launch<true, 2, 1>(a, n, s); break;
        case 130: launch<true, 2, 2>(a, n, s); break;
        case 131: launch<true, 2, 3>(a, n, s); break;
        default: return hipErrorNotSupported;
    }
    return hipGetLastError();
}
