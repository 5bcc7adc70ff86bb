// Pieces of the split-bf16 volume kernel (volume_split.hip): the LDS-DMA
// ring's geometry and a lane's fragment read + split.
#pragma once
#include "common.h"
#include "epilogue.h"
#include "split.h"

namespace rc {

constexpr int kSpBK = 16;                   // d per ring stage (two per K step)
constexpr int kSpMaxFused = 5;              // levels the epilogue writes (more: pooled from memory)

// Ring geometry for stage rows TW floats wide (the tile width in w: 128) and
// SL slots (stages).  SL 4: two whole K steps, one in use, the other in
// flight, refilled a K step at a time at the top of a step.
// SL 3: one K step in use plus ONE stage in flight; the two slots a K step
// read are refilled in the middle of that step, behind a second workgroup
// barrier after the waves' last fragment read (split_body).  A DMA block
// holds two rows (2 TW fp32 = TW / 2 lanes x 16 B) plus 16 B of padding, so
// rows d and d + 8 (4 blocks apart) fall on different ds_read_b32 banks:
// 4 (8 TW + 16) / 4 = 16 mod 32 dwords for TW % 16 == 0.
//   TW 128, SL 4: 66.5 KB -- two workgroups per CU;
//   TW 128, SL 3: 48.75 KB -- three workgroups per CU (DESIGN.md §3.1c for
//   which shapes run which).
// Rows 80 wide with 6 / 4 slots were measured and not kept.
template <int TW, int SL>
struct SpRing {
    static_assert(TW == 128 && (SL == 3 || SL == 4), "split ring geometry");
    static constexpr int Blk = 8 * TW + 16;   // bytes per DMA block: 2 rows + 16 B pad
    static constexpr int Op = 8 * Blk;        // one operand tile of a stage: 16 rows
    static constexpr int Slot = 2 * Op;       // F1 + F2
    static constexpr int Bytes = SL * Slot;
    static constexpr int Wave = Bytes / 4;    // per-wave epilogue staging once the ring drains
    static constexpr int KA = SL / 2;         // whole K steps the ring holds (SL 3: one, plus a stage)
    static constexpr int Pro = SL == 3 ? 3 : 2 * KA;   // stages the prologue issues
};
constexpr int kSpStb = 16 * (64 + 4) * 4;     // per-wave epilogue staging (epilogue_swapped, WT 64)
static_assert(kSpStb <= SpRing<128, 3>::Wave, "epilogue staging aliases the ring");

// One lane's fragment: rows r0..r0+7 (d inside the stage) of w column w of an
// operand tile at LDS byte address base.  Row d of the tile sits in block
// d >> 1 at +4 TW bytes for odd d.
template <int TW = 128>
__device__ __forceinline__ void sp_read_raw(const char *base, float (&x)[8]) {
    constexpr int Blk = SpRing<TW, 4>::Blk;
#pragma unroll
    for (int j = 0; j < 8; ++j) x[j] = *reinterpret_cast<const float *>(base + (j >> 1) * Blk + (j & 1) * 4 * TW);
}
template <int MODE>
__device__ __forceinline__ SplitFrag sp_split_raw(const float (&x)[8]) {
    if constexpr (MODE & kModeNoSplit) {     // dev timing probe: head piece only, reused thrice
        u32x4s h;
#pragma unroll
        for (int k = 0; k < 4; ++k) h[k] = sp_pack(x[2 * k], x[2 * k + 1]);
        const bf16x8 hb = __builtin_bit_cast(bf16x8, h);
        return SplitFrag{hb, hb, hb};
    }
    return sp_split(x);
}
template <int MODE, int TW = 128>
__device__ __forceinline__ SplitFrag sp_read(const char *base) {
    float x[8];
    sp_read_raw<TW>(base, x);
    return sp_split_raw<MODE>(x);
}

}  // namespace rc
