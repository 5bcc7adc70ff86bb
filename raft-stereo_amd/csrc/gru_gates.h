// What the ConvGRU glue kernels share (gru_gates.hip: forward,
// gru_gates_bwd.hip: backward): the per-element sigmoid, the V-element access,
// the choice of the access width and the launch shape.  The header comment of
// gru_gates.hip describes the operand model.
#pragma once
#include "lookup_pair.h"   // out_cvt: the opaque copy keeps the last fp32 op and the convert two roundings

namespace rc {

__device__ __forceinline__ float gru_sigmoid(float a) {
    const float e = __builtin_amdgcn_exp2f(-a * 1.44269504088896340736f);
    return __builtin_amdgcn_rcpf(1.0f + e);
}

template <class T, int V>
struct alignas(sizeof(T) * V) GruPack {
    T v[V];
};

template <class T, int V>
__device__ __forceinline__ GruPack<T, V> gru_load(const GruOperand &op, long long n, long long o, long long i) {
    return *reinterpret_cast<const GruPack<T, V> *>(static_cast<const T *>(op.p) + n * op.sn + o * op.so + i);
}

template <class T, int V>
__device__ __forceinline__ void gru_store(const GruOperand &op, long long n, long long o, long long i,
                                          const GruPack<T, V> &v) {
    *reinterpret_cast<GruPack<T, V> *>(static_cast<T *>(op.p) + n * op.sn + o * op.so + i) = v;
}

// Largest access width (bytes: 16, 8 or one element) that the inner length,
// every base address and every stride are whole multiples of.  A: GruArgs or
// GruBwdArgs.
template <class A>
static int gru_width(const A &a, int nops, int esize) {
    for (int bytes = 16; bytes > esize; bytes >>= 1) {
        const long long v = bytes / esize;
        bool ok = a.L % v == 0;
        for (int k = 0; k < nops && ok; ++k)
            ok = reinterpret_cast<uintptr_t>(a.op[k].p) % (uintptr_t)bytes == 0 && a.op[k].sn % v == 0 &&
                 a.op[k].so % v == 0;
        if (ok) return bytes;
    }
    return esize;
}

// Sets the unit counts of `a` for V elements per unit; returns the capped
// one-dimensional grid of 256-thread workgroups, the rest is the kernels'
// grid-stride loop.
template <class A>
static dim3 gru_grid(A &a, int V) {
    const long long units = (long long)a.N * a.O * (a.L / V);
    a.J = (uint32_t)(a.L / V);
    a.units = (uint32_t)units;
    const long long cap = (long long)device_cus() * 8, need = (units + 255) / 256;
    return dim3((unsigned)(need < cap ? need : cap));
}

}  // namespace rc
