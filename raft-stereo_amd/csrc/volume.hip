// Correlation volume + fused pyramid epilogue, fp32 MFMA (gfx950).
//
// Replaces CorrBlock1D.corr (/root/reference/model.py:318-326) and the
// avg_pool2d loop of CorrBlock1D.__init__ (:284-295).
//
// Per (b,h) image row the volume is a GEMM  C[w1][w2] = sum_d F1[d][w1] F2[d][w2]
// with K = D.  F1/F2 are NCHW, so for a fixed row both operands are "K-major":
// row d of an operand is W contiguous floats.  v_mfma_f32_16x16x4_f32 takes one
// f32 per lane for A and for B: lane l supplies A[i=l&15][k=l>>4] and
// B[k=l>>4][j=l&15].  A lane loads FM (A) or 4 (B) consecutive floats along w
// (16 lanes cover one contiguous d-row segment, the wave 4 d-rows); component
// c of that vector is the operand of the c-th of FM (or 4) 16-wide fragments
// whose rows are w = w0 + FM*i + c.  The output is therefore interleaved:
// fragment (ma,nb) register r of lane l holds
//     C[m0 + FM*((l>>4)*4 + r) + ma][n0 + 4*(l&15) + nb].
// Each lane thus owns 4 consecutive w2 of a row, which makes the first two
// pooling steps lane-local and the next ones xor-shuffles (l^1, l^2, ...).
//
// Workgroup: 256 threads = 4 waves in a 2x2 arrangement of 64x64 wave tiles
// (a 128x128 tile of one row's volume).  A wave whose tile has fewer than 64
// valid w1 rows uses FM = ceil(rows/16) fragments (e.g. 3 for the 48-row tail
// of W1 = 240), so padding costs at most 15 rows of MFMA work.  Workgroups are
// remapped so all tiles of one (b,h) row run on one XCD (blocks b, b+8, ...
// share an XCD) and share that XCD's L2 copy of the row's feature maps.
//
// K loop: two named register sets (no copies, static indexing) each holding U
// k-steps; one set is loading while the other feeds the MFMAs.  K steps past D
// load zeros (buffer offset pushed out of range), so there are no per-step
// guards.
#include "common.h"
#include "epilogue.h"
#include "volume_b16.h"   // store_staged, epilogue; the bf16 MFMA kernels

namespace rc {

template <int N>
struct FragVec;
template <>
struct FragVec<4> { typedef f32x4 T; };
template <>
struct FragVec<3> { typedef float T __attribute__((ext_vector_type(3))); };
template <>
struct FragVec<2> { typedef f32x2 T; };
template <>
struct FragVec<1> { typedef float T __attribute__((ext_vector_type(1))); };

// Load N consecutive floats along w at (d, w) of one image, zeros when d >= D.
template <int N, bool VEC>
__device__ __forceinline__ typename FragVec<N>::T load_frag(__amdgpu_buffer_rsrc_t r, int d, int D,
                                                            int H, int h, int W, int w) {
    typedef typename FragVec<N>::T V;
    uint32_t off = (uint32_t)(((long long)(d * H + h) * W + w) * 4);
    if (d >= D) off = 0xFFFFFF00u;
    V v;
    if constexpr (VEC && N == 4) {
        v = ld4(r, off);
    } else if constexpr (VEC && N == 3) {
        v = __builtin_bit_cast(V, __builtin_amdgcn_raw_buffer_load_b96(r, (int)off, 0, 0));
    } else if constexpr (VEC && N == 2) {
        v = __builtin_bit_cast(V, __builtin_amdgcn_raw_buffer_load_b64(r, (int)off, 0, 0));
    } else {
#pragma unroll
        for (int c = 0; c < N; ++c) v[c] = ld1(r, off + 4 * c);
    }
    return v;
}

template <int FM, int U>
struct Stage {
    typename FragVec<FM>::T a[U];
    f32x4 b[U];
};

template <int FM, int U, bool VEC, int MODE>
__device__ __forceinline__ void load_stage(Stage<FM, U> &s, int k0, int kd,
                                           __amdgpu_buffer_rsrc_t r1, __amdgpu_buffer_rsrc_t r2,
                                           int D, int H, int h, int W1, int W2, int wa, int wb) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
        if constexpr (MODE & kModeNoLoads) {
#pragma unroll
            for (int c = 0; c < FM; ++c) s.a[u][c] = (float)(wa + c + u) * 1e-3f;
            s.b[u] = f32x4{(float)wb, (float)(wb + 1), (float)(k0 + u), 1.0f} * 1e-3f;
        } else {
            s.a[u] = load_frag<FM, VEC>(r1, k0 + 4 * u + kd, D, H, h, W1, wa);
            s.b[u] = load_frag<4, VEC>(r2, k0 + 4 * u + kd, D, H, h, W2, wb);
        }
    }
}

template <int FM, int U>
__device__ __forceinline__ void mma_stage(const Stage<FM, U> &s, f32x4 (&acc)[FM][4]) {
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
        for (int ma = 0; ma < FM; ++ma)
#pragma unroll
            for (int nb = 0; nb < 4; ++nb)
                acc[ma][nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(s.a[u][ma], s.b[u][nb],
                                                                   acc[ma][nb], 0, 0, 0);
}

template <int FM, int U, bool VEC, int MODE>
__device__ __forceinline__ void wave_tile(const BuildArgs &a, int row, int b, int h, int m0,
                                          int n0, int lane, float *stA, float *stB) {
    const int D = a.D, H = a.H, W1 = a.W1, W2 = a.W2;
    const long long img1 = (long long)D * H * W1, img2 = (long long)D * H * W2;
    const auto r1 = make_rsrc(reinterpret_cast<const float *>(a.f1) + b * img1, clamp_bytes(img1 * 4));
    const auto r2 = make_rsrc(reinterpret_cast<const float *>(a.f2) + b * img2, clamp_bytes(img2 * 4));
    const int kd = lane >> 4;             // d offset inside a k-step
    const int wa = m0 + FM * (lane & 15); // this lane's w1 group
    const int wb = n0 + 4 * (lane & 15);  // this lane's w2 quad

    f32x4 acc[FM][4];
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    constexpr int KS = 4 * U;                      // d per stage
    const int nst = (D + KS - 1) / KS;             // stages (tail stages read zeros)
    Stage<FM, U> s0, s1;
    load_stage<FM, U, VEC, MODE>(s0, 0, kd, r1, r2, D, H, h, W1, W2, wa, wb);
    load_stage<FM, U, VEC, MODE>(s1, KS, kd, r1, r2, D, H, h, W1, W2, wa, wb);
    for (int st = 0; st < nst; st += 2) {
        mma_stage<FM, U>(s0, acc);
        if (st + 2 < nst) load_stage<FM, U, VEC, MODE>(s0, (st + 2) * KS, kd, r1, r2, D, H, h, W1, W2, wa, wb);
        if (st + 1 < nst) {
            mma_stage<FM, U>(s1, acc);
            if (st + 3 < nst) load_stage<FM, U, VEC, MODE>(s1, (st + 3) * KS, kd, r1, r2, D, H, h, W1, W2, wa, wb);
        }
    }

    epilogue<FM, MODE, false>(acc, a, row, m0, n0, lane, stA, stB);
}

template <bool VEC, int U, int MODE>
__global__ __launch_bounds__(256) void build_f32_kernel(BuildArgs a, int nwg_total) {
    // one LDS array (guide §5 trap 4a): per wave an 8 KB + 4 KB ping-pong
    // staging image for the pooled levels
    __shared__ __attribute__((aligned(16))) float smem[4][kStageFloats + kStageFloats / 2];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float *stA = smem[wave], *stB = smem[wave] + kStageFloats;
    const int T = a.tiles_m * a.tiles_n;
    auto tile_body = [&](int v) {
        const int wgid = xcd_remap(v, nwg_total);
        const int row = wgid / T, tile = wgid - row * T;
        const int tm = tile / a.tiles_n, tn = tile - tm * a.tiles_n;
        const int b = row / a.H, h = row - b * a.H;
        const int m0 = tm * 128 + (wave >> 1) * 64;
        const int n0 = tn * 128 + (wave & 1) * 64;
        if (m0 >= a.W1 || n0 >= a.W2) return;   // wave-uniform; no barriers in this kernel
        const int rows = a.W1 - m0;             // valid w1 rows of this wave tile
        if (rows > 48)
            wave_tile<4, U, VEC, MODE>(a, row, b, h, m0, n0, lane, stA, stB);
        else if (rows > 32)
            wave_tile<3, U, VEC, MODE>(a, row, b, h, m0, n0, lane, stA, stB);
        else if (rows > 16)
            wave_tile<2, U, VEC, MODE>(a, row, b, h, m0, n0, lane, stA, stB);
        else
            wave_tile<1, U, VEC, MODE>(a, row, b, h, m0, n0, lane, stA, stB);
    };
    tile_body(blockIdx.x);
}

// ============ fp32 MFMA with a workgroup LDS-DMA ring (default) ============
//
// Operand tiles are shared by the workgroup's four waves through a 3-slot LDS
// ring filled by buffer->LDS DMA (buffer_load_dwordx4 ... lds): slot = a
// [16 d][128 w] tile of F1 and of F2 (16 KB), two stages in flight ahead of
// the one being multiplied, no VGPR staging.  Stage s+2 is issued into the
// slot stage s-1 used, after the barrier that follows every wave's counted
// vmcnt for stage s (RAW) and its lgkmcnt(0) for the reads of stage s-1
// (WAR) -- cdna_hip_programming.md §5 "Pipelining across barriers".
// Fragments are read with ds_read_b128 (conflict-free: the 16-lane groups of
// a b128 read cover all 64 banks of two 512-B rows).  Waves with no valid
// rows still issue their share of the DMA and join every barrier.
constexpr int kRingSlots = 3;
constexpr int kBK = 16;                       // d rows per ring stage
constexpr int kSlotFloats = 2 * kBK * 128;    // A + B tiles of one stage
static_assert(kRingSlots * kSlotFloats >= 4 * (kStageFloats + kStageFloats / 2),
              "epilogue staging must fit in the ring");

template <int FM, int FN>
__device__ __forceinline__ void ring_stage(const float *sA, const float *sB, int am, int bn,
                                           int lane, f32x4 (&acc)[FM][4]) {
#pragma unroll
    for (int kk = 0; kk < kBK / 4; ++kk) {
        const int dr = 4 * kk + (lane >> 4);
        const float *pa = sA + dr * 128 + am + FM * (lane & 15);
        float av[4], bv[4];
        if constexpr (FM == 4) {
            const f32x4 v = *reinterpret_cast<const f32x4 *>(pa);
            av[0] = v[0]; av[1] = v[1]; av[2] = v[2]; av[3] = v[3];
        } else if constexpr (FM == 2) {
            const f32x2 v = *reinterpret_cast<const f32x2 *>(pa);
            av[0] = v[0]; av[1] = v[1];
        } else {
#pragma unroll
            for (int c = 0; c < FM; ++c) av[c] = pa[c];
        }
        const float *pb = sB + dr * 128 + bn + FN * (lane & 15);
        if constexpr (FN == 4) {
            const f32x4 v = *reinterpret_cast<const f32x4 *>(pb);
            bv[0] = v[0]; bv[1] = v[1]; bv[2] = v[2]; bv[3] = v[3];
        } else {
#pragma unroll
            for (int c = 0; c < FN; ++c) bv[c] = pb[c];
        }
#pragma unroll
        for (int ma = 0; ma < FM; ++ma)
#pragma unroll
            for (int nb = 0; nb < FN; ++nb)
                acc[ma][nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[ma], bv[nb], acc[ma][nb], 0, 0, 0);
    }
}

struct RingCtx {
    __amdgpu_buffer_rsrc_t r1, r2;
    int D, H, h, W1, W2, M0, N0, wave, lane, nst;
};

// DMA share of this wave per stage: rows 4w..4w+3 of both tiles, 2 rows
// (1 KB = 64 lanes x 16 B) per instruction -> 4 instructions per stage.
template <int SL>
__device__ __forceinline__ void ring_issue(const RingCtx &c, float *smem, int st) {
    typedef __attribute__((address_space(3))) void lds_void;
    float *sA = smem + (st % SL) * kSlotFloats, *sB = sA + kBK * 128;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int r0 = 4 * c.wave + 2 * i;
        const int d = st * kBK + r0 + (c.lane >> 5);
        const int w = 4 * (c.lane & 31);
        const long long base = (long long)(d < c.D ? d : 0) * c.H + c.h;
        const uint32_t offA = d < c.D ? (uint32_t)((base * c.W1 + c.M0 + w) * 4) : 0xFFFFFF00u;
        const uint32_t offB = d < c.D ? (uint32_t)((base * c.W2 + c.N0 + w) * 4) : 0xFFFFFF00u;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(c.r1, (lds_void *)(sA + r0 * 128), 16, (int)offA, 0, 0, 0);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(c.r2, (lds_void *)(sB + r0 * 128), 16, (int)offB, 0, 0, 0);
    }
}

// The whole K loop + epilogue for one wave with FM A-fragments and FN
// B-fragments (FM = 0: a wave with no valid rows -- it still issues its DMA
// share and joins every barrier, so all four waves execute the same barrier
// sequence).
template <int FM, int FN, int MODE, int SL>
__device__ __forceinline__ void ring_body(const RingCtx &c, const BuildArgs &a, float *smem, int row,
                                          int am, int bn) {
    f32x4 acc[FM > 0 ? FM : 1][4];
#pragma unroll
    for (int i = 0; i < (FM > 0 ? FM : 1); ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < SL - 1; ++s)
        if (s < c.nst) ring_issue<SL>(c, smem, s);
    for (int st = 0; st < c.nst; ++st) {
        // RAW: my DMA for stage st landed (the later stages' 4 instructions
        // each may stay in flight); WAR: my LDS reads of stage st-1 are done.
        // Then the barrier.
        const int later = min(SL - 2, c.nst - 1 - st);
        if (later >= 3) asm volatile("s_waitcnt vmcnt(12) lgkmcnt(0)" ::: "memory");
        else if (later == 2) asm volatile("s_waitcnt vmcnt(8) lgkmcnt(0)" ::: "memory");
        else if (later == 1) asm volatile("s_waitcnt vmcnt(4) lgkmcnt(0)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        if (st + SL - 1 < c.nst) ring_issue<SL>(c, smem, st + SL - 1);
        if constexpr (FM > 0) {
            const float *sA = smem + (st % SL) * kSlotFloats, *sB = sA + kBK * 128;
            ring_stage<FM, FN>(sA, sB, am, bn, c.lane, acc);
        }
    }
    // everyone is done with the ring before it becomes epilogue staging
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if constexpr (FM > 0) {
        float *stA = smem + c.wave * (kStageFloats + kStageFloats / 2), *stB = stA + kStageFloats;
        epilogue<FM, MODE, false>(acc, a, row, c.M0 + am, c.N0 + bn, c.lane, stA, stB);
    }
}

// FN = 4 B-fragments: 64-wide wave tiles, WG 128x128.  (48-wide tiles with
// FN = 3, which avoid padding at W = 240/720, measured slower: 414 vs 372 us
// at config 2 -- more workgroups re-read A and the B DMA/FLOP grows.)
template <int FN, int MODE, int SL = kRingSlots>
__global__ __launch_bounds__(256) void build_f32_ring_kernel(BuildArgs a, int nwg_total) {
    static_assert(SL >= 3 && SL <= 5, "ring depth");
    __shared__ __attribute__((aligned(16))) float smem[SL * kSlotFloats];
    RingCtx c;
    c.wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    c.lane = threadIdx.x & 63;
    const int T = a.tiles_m * a.tiles_n;
    const int wgid = xcd_remap(blockIdx.x, nwg_total);
    const int row = wgid / T, tile = wgid - row * T;
    const int tm = tile / a.tiles_n, tn = tile - tm * a.tiles_n;
    const int b = row / a.H;
    c.h = row - b * a.H;
    c.D = a.D; c.H = a.H; c.W1 = a.W1; c.W2 = a.W2;
    c.M0 = tm * 128; c.N0 = tn * 32 * FN;
    c.nst = (a.D + kBK - 1) / kBK;
    const long long img1 = (long long)a.D * a.H * a.W1, img2 = (long long)a.D * a.H * a.W2;
    c.r1 = make_rsrc(reinterpret_cast<const float *>(a.f1) + b * img1, clamp_bytes(img1 * 4));
    c.r2 = make_rsrc(reinterpret_cast<const float *>(a.f2) + b * img2, clamp_bytes(img2 * 4));
    const int am = (c.wave >> 1) * 64, bn = (c.wave & 1) * 16 * FN;   // wave tile in the WG tile
    const int m0 = c.M0 + am, n0 = c.N0 + bn;
    const int rows = a.W1 - m0;
    const bool active = rows > 0 && n0 < a.W2;                         // wave-uniform
    if (!active) ring_body<0, FN, MODE, SL>(c, a, smem, row, am, bn);
    else if (rows > 48) ring_body<4, FN, MODE, SL>(c, a, smem, row, am, bn);
    else if (rows > 32) ring_body<3, FN, MODE, SL>(c, a, smem, row, am, bn);
    else if (rows > 16) ring_body<2, FN, MODE, SL>(c, a, smem, row, am, bn);
    else ring_body<1, FN, MODE, SL>(c, a, smem, row, am, bn);
}

template <bool VEC, int U, int MODE>
static void launch(const BuildArgs &a, unsigned nwg, hipStream_t s) {
    hipLaunchKernelGGL((build_f32_kernel<VEC, U, MODE>), dim3(nwg), dim3(256), 0, s, a, (int)nwg);
}

template <int MODE, int SL = kRingSlots>
static void launch_ring(const BuildArgs &a, hipStream_t s) {
    const long long nwg = (long long)a.B * a.H * a.tiles_m * a.tiles_n;
    if (nwg <= 0 || nwg > 0x7FFFFFFF) return;
    hipLaunchKernelGGL((build_f32_ring_kernel<4, MODE, SL>), dim3((unsigned)nwg), dim3(256), 0, s, a, (int)nwg);
}

#ifdef RAFTCORR_DEV
#include "dev/volume_dev.inc"   // ablation modes and measured variants: libraftcorr_dev.so only
#endif

template <bool IN_BF16, bool ALIGNED>
static void launch_bf16(const BuildArgs &a, unsigned nwg, hipStream_t s) {
#ifdef RAFTCORR_DEV
    if (dev_launch_bf16_pw<IN_BF16, ALIGNED>(a, nwg, s)) return;
#endif
    hipLaunchKernelGGL((build_bf16_kernel<IN_BF16, ALIGNED, 0>), dim3(nwg), dim3(256), 0, s, a, (int)nwg);
}

}  // namespace rc

// bf16 MFMA build.  The ring kernel fuses at most kB16MaxFused levels:
// a.nfused is lowered to what was written, and the caller pools the rest.
hipError_t rc_launch_build_bf16mma(rc::BuildArgs &a, int in_bf16, hipStream_t s) {
    if (a.pyr_bf16 == rc::kF16) return rc_launch_build_f16mma(a, in_bf16, s);   // volume_half.hip
    const long long nwg = (long long)a.B * a.H * a.tiles_m * a.tiles_n;
    if (nwg <= 0) return hipSuccess;
    if (nwg > 0x7FFFFFFF) return hipErrorInvalidValue;
    const unsigned n = (unsigned)nwg;
    if (a.rec) {
        // RC_LAYOUT_RECORDS: the deferred ring kernel with one tile across
        // the whole row (NWN = ceil(W2 / 64) waves along w2) and at least
        // 8 stages per tile (its four pieces take two stages each)
        const int nwn = (a.W2 + 63) / 64;
        if (!in_bf16 || !a.pyr_bf16 || nwn < 2 || a.W2 > rc::kRecMaxW2 || (a.D + rc::kB16BK - 1) / rc::kB16BK < 8 ||
            (long long)a.D * a.H * (a.W1 > a.W2 ? a.W1 : a.W2) * 2 >= (1LL << 30))
            return hipErrorNotSupported;
        constexpr int RM = rc::kModeRecords;
#ifdef RAFTCORR_DEV
        if (const hipError_t e = rc::dev_launch_records(a, nwn, s); e != hipErrorNotSupported) return e;
#endif
        if (nwn == 5) rc::launch_bf16_ring_n<5, 4, 4, RM, true>(a, s);
        else if (nwn == 4) rc::launch_bf16_ring_n<4, 4, 4, RM, true>(a, s);
        else if (nwn == 3) rc::launch_bf16_ring_n<3, 4, 4, RM, true>(a, s);
        else rc::launch_bf16_ring_n<2, 4, 4, RM, true>(a, s);
        return hipGetLastError();
    }
    rc::B16Shape sh = in_bf16 ? rc::bf16_ring_shape(a) : rc::B16Shape{0, 0, false};
#ifdef RAFTCORR_DEV
    if (const hipError_t e = rc::dev_launch_bf16mma(a, sh, s); e != hipErrorNotSupported) return e;
#endif
    if (sh.nwn) {
        if (a.nfused > rc::kB16MaxFused) a.nfused = rc::kB16MaxFused;
        rc::launch_bf16_ring<0>(a, sh, s);
        return hipGetLastError();
    }
    if (in_bf16) {
        if (a.W1 % 8 == 0 && a.W2 % 8 == 0) rc::launch_bf16<true, true>(a, n, s);
        else rc::launch_bf16<true, false>(a, n, s);
    } else {
        if (a.W1 % 4 == 0 && a.W2 % 4 == 0) rc::launch_bf16<false, true>(a, n, s);
        else rc::launch_bf16<false, false>(a, n, s);
    }
    return hipGetLastError();
}

// The exact fp32 MFMA build (LDS-DMA ring kernel, 3 slots).
hipError_t rc_launch_build_f32(const rc::BuildArgs &a, hipStream_t s) {
    const long long nwg = (long long)a.B * a.H * a.tiles_m * a.tiles_n;
    if (nwg <= 0) return hipSuccess;
    if (nwg > 0x7FFFFFFF) return hipErrorInvalidValue;
    const bool vec = (a.W1 % 4 == 0) && (a.W2 % 4 == 0);
    const unsigned n = (unsigned)nwg;
    if (!vec) {
        rc::launch<false, 2, 0>(a, n, s);
        return hipGetLastError();
    }
#ifdef RAFTCORR_DEV
    if (const hipError_t e = rc::dev_launch_f32(a, n, s); e != hipErrorNotSupported) return e;
#endif
    rc::launch_ring<0>(a, s);
    return hipGetLastError();
}
