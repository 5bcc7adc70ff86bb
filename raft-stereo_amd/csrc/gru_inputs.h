// What the ConvGRU input assembly (gru_inputs.hip) and its adjoint
// (gru_inputs_bwd.hip) share: the global-memory accesses, the bilinear axis
// (one definition: the backward's weights are the forward's), the clamp, the
// opaque trip count and the moves into scalar registers.
#pragma once
#include "gru_gates.h"    // GruPack, out_cvt, device_cus

namespace rc {

// A source pointer as a global-memory one: a descriptor that went through
// scalar registers (asm_scalar) no longer tells the compiler, which would
// fall back to flat loads.
#ifdef __HIP_DEVICE_COMPILE__
#define ASM_GLOBAL __attribute__((address_space(1)))
#else
#define ASM_GLOBAL      // the host pass only parses the kernels
#endif
template <class S>
__device__ __forceinline__ const ASM_GLOBAL S *asm_global(const void *p) {
    return (const ASM_GLOBAL S *)reinterpret_cast<uintptr_t>(p);
}

template <class S>
__device__ __forceinline__ float asm_ld1(const void *p, long long off) {
    return (float)asm_global<S>(p)[off];
}

// V consecutive elements of type S as they are: one access of up to 16 bytes
template <class S, int V>
__device__ __forceinline__ GruPack<S, V> asm_ldv(const void *p, long long off) {
    static_assert(sizeof(S) * V <= 16, "one access");
    return *(const ASM_GLOBAL GruPack<S, V> *)(asm_global<S>(p) + off);
}

struct AsmAxis {
    int i0, i1;
    float l0, l1;
};
__device__ __forceinline__ AsmAxis asm_axis(float scale, int i, int S) {
    const float s = scale * (float)i;
    int i0 = (int)s;
    i0 = i0 < S - 1 ? i0 : S - 1;
    AsmAxis x;
    x.i0 = i0;
    x.i1 = i0 + (i0 < S - 1 ? 1 : 0);
    x.l1 = s - (float)i0;
    x.l0 = 1.0f - x.l1;
    return x;
}

__device__ __forceinline__ int asm_clamp(int i, int S) { return i < 0 ? 0 : (i < S ? i : S - 1); }

// V behind an opaque copy: the planar gather loops stay rolled (a loop of a
// known short trip count is unrolled whatever the pragma says).
template <int V>
__device__ __forceinline__ int asm_trips() {
    int v = V;
    asm volatile("" : "+s"(v));
    return v;
}

// A descriptor picked by a wave-uniform index, moved to scalar registers (the
// compiler loads a dynamically indexed kernel argument per lane).
__device__ __forceinline__ int asm_s(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ long long asm_s(long long v) {
    const unsigned lo = (unsigned)asm_s((int)(unsigned)v), hi = (unsigned)asm_s((int)((unsigned long long)v >> 32));
    return (long long)((unsigned long long)hi << 32 | lo);
}
__device__ __forceinline__ float asm_s(float v) {
    return __builtin_bit_cast(float, asm_s(__builtin_bit_cast(int, v)));
}

}  // namespace rc
