// The input assembly of a ConvGRU update (network.py, BasicMultiUpdateBlock):
// the [h, x] buffer filled by one memory-bound launch (rc_gru_assemble; gfx950)
// from up to kGruMaxParts sources, each written into its own channel range:
//   copy      dst = (T)src                         the torch.cat copy and its cast
//   pool2x    3x3 average, stride 2, zero padding 1, padding counted   (pool2x)
//   bilinear  resize with align_corners=True                           (interp)
// The pooled and the resized tensors are never in memory.
//
// dst is planar (column stride 1) or interleaved (channel stride 1); a source
// has any four element strides.  A work unit is V elements of dst along its
// unit-stride axis, stored as one access of V * sizeof(T) bytes: V channels of
// one pixel (interleaved) or V columns of one row of one channel (planar).  16
// bytes where every base, stride and length allows, else 8, else one element
// (asm_fits chooses).  With V > 1 an interleaved unit reads each of its source
// pixels (one, nine or four) as one V-wide access, so every source has channel
// stride 1 there; a planar unit reads a copied source as one V-wide access
// (column stride 1) and gathers the pooled and resized ones element by element
// from rows that neighbouring lanes share.  The part of a unit follows from
// its channel; a wave takes the parts its units belong to one after the other
// (most waves lie within one), each with the descriptor in scalar registers.
//
// Arithmetic: fp32 on the widened inputs, each operation rounded on its own
// (-ffp-contract=off), one rounding to T at the store (out_cvt); the same
// per-element sequence in every instance, so planar, interleaved and every
// width give the same bits.
//   pool2x:   sum of the window's in-image taps, row by row from 0.0f, then
//             / 9.0f (correctly rounded).  A tap outside the image adds 0.0f:
//             its load goes to a clamped (in-image) address so that it can
//             be issued without a branch, and a select discards what it read.
//             The sum is never -0.0f after its first addition, so adding
//             0.0f leaves its bits.
//   bilinear: ATen's sequence.  s = scale * i, i0 = (int)s, i1 = i0 + (i0 < S-1),
//             l1 = s - i0, l0 = 1 - l1; l0h*(l0w*a + l1w*b) + l1h*(l0w*c + l1w*d).
//             i0 is clamped to S - 1 (it never exceeds it by the formula; the
//             clamp keeps every address in the image whatever scale holds).
#include "gru_inputs.h"  // asm_ld1, asm_ldv, asm_axis, asm_clamp, asm_trips, asm_s

namespace rc {

// o as a shift register: element k of a planar unit enters at the top in pass
// k of a rolled loop, so after V passes it sits at index k.  Static indices
// only (a run-time index would put o in scratch), and one window's gathers
// and addresses in registers at a time whatever V is.
template <class T, int V>
__device__ __forceinline__ void asm_push(GruPack<T, V> &o, float v) {
#pragma unroll
    for (int k = 0; k + 1 < V; ++k) o.v[k] = o.v[k + 1];
    asm("" : "+v"(v));      // as out_cvt does for the 16-bit types: the passes stay one loop for fp32 too
    o.v[V - 1] = out_cvt<T>(v);
}

// One unit of part P, whose source holds elements of type S.  Interleaved:
// channels c .. c+V-1 of pixel (h, w); planar: columns w .. w+V-1 of row h of
// channel c.
template <class T, class S, int V, bool INTER>
__device__ __forceinline__ void asm_unit_t(const GruPart &P, int n, int c, int h, int w, GruPack<T, V> &o) {
    const long long b = (long long)n * P.sn + (long long)(c - P.c0) * P.sc;
    if (P.mode == kPartCopy) {
        const GruPack<S, V> t = asm_ldv<S, V>(P.p, b + (long long)h * P.sh + (long long)w * P.sw);
#pragma unroll
        for (int k = 0; k < V; ++k) o.v[k] = out_cvt<T>((float)t.v[k]);
    } else if (P.mode == kPartPool2x) {
        if constexpr (INTER) {
            float acc[V];
#pragma unroll
            for (int k = 0; k < V; ++k) acc[k] = 0.0f;
#pragma unroll 1
            for (int kh = 0; kh < 3; ++kh) {
                const int ih = 2 * h - 1 + kh;
                const bool okh = ih >= 0 && ih < P.SH;
                const long long br = b + (long long)asm_clamp(ih, P.SH) * P.sh;
                GruPack<S, V> t[3];
#pragma unroll
                for (int kw = 0; kw < 3; ++kw)
                    t[kw] = asm_ldv<S, V>(P.p, br + (long long)asm_clamp(2 * w - 1 + kw, P.SW) * P.sw);
#pragma unroll
                for (int kw = 0; kw < 3; ++kw) {
                    const int iw = 2 * w - 1 + kw;
                    const bool ok = okh && iw >= 0 && iw < P.SW;
#pragma unroll
                    for (int k = 0; k < V; ++k) acc[k] = acc[k] + (ok ? (float)t[kw].v[k] : 0.0f);
                }
            }
#pragma unroll
            for (int k = 0; k < V; ++k) o.v[k] = out_cvt<T>(acc[k] / 9.0f);
        } else {
#pragma unroll 1
            for (int k = 0, trips = asm_trips<V>(); k < trips; ++k) {
                const int iw = 2 * (w + k) - 1;       // the window's first column; every address is clamped into the row
                const bool ok0 = iw >= 0, ok1 = iw + 1 < P.SW, ok2 = iw + 2 < P.SW;
                const long long c0 = (long long)asm_clamp(iw, P.SW) * P.sw, c1 = (long long)asm_clamp(iw + 1, P.SW) * P.sw;
                const long long c2 = (long long)asm_clamp(iw + 2, P.SW) * P.sw;
                float acc = 0.0f;
#pragma unroll
                for (int kh = 0; kh < 3; ++kh) {
                    const int ih = 2 * h - 1 + kh;
                    const long long br = b + (long long)asm_clamp(ih, P.SH) * P.sh;
                    const float t0 = asm_ld1<S>(P.p, br + c0), t1 = asm_ld1<S>(P.p, br + c1);
                    const float t2 = asm_ld1<S>(P.p, br + c2);
                    // a row outside the image adds three zeros: the sum keeps its bits
                    float row = acc + (ok0 ? t0 : 0.0f);
                    row = row + (ok1 ? t1 : 0.0f);
                    row = row + (ok2 ? t2 : 0.0f);
                    acc = ih >= 0 && ih < P.SH ? row : acc;
                }
                asm_push<T, V>(o, acc / 9.0f);
            }
        }
    } else {
        const AsmAxis y = asm_axis(P.scale_h, h, P.SH);
        const long long r0 = b + (long long)y.i0 * P.sh, r1 = b + (long long)y.i1 * P.sh;
        if constexpr (INTER) {
            const AsmAxis x = asm_axis(P.scale_w, w, P.SW);
            const long long c0 = (long long)x.i0 * P.sw, c1 = (long long)x.i1 * P.sw;
            const GruPack<S, V> ta = asm_ldv<S, V>(P.p, r0 + c0), tb = asm_ldv<S, V>(P.p, r0 + c1);
            const GruPack<S, V> tc = asm_ldv<S, V>(P.p, r1 + c0), td = asm_ldv<S, V>(P.p, r1 + c1);
#pragma unroll
            for (int k = 0; k < V; ++k) {
                const float top = x.l0 * (float)ta.v[k] + x.l1 * (float)tb.v[k];
                const float bot = x.l0 * (float)tc.v[k] + x.l1 * (float)td.v[k];
                o.v[k] = out_cvt<T>(y.l0 * top + y.l1 * bot);
                if (k % 2 == 1) __builtin_amdgcn_sched_barrier(0);     // widen two elements at a time
            }
        } else {
#pragma unroll 1
            for (int k = 0, trips = asm_trips<V>(); k < trips; ++k) {
                const AsmAxis x = asm_axis(P.scale_w, w + k, P.SW);
                const long long c0 = (long long)x.i0 * P.sw, c1 = (long long)x.i1 * P.sw;
                const float ta = asm_ld1<S>(P.p, r0 + c0), tb = asm_ld1<S>(P.p, r0 + c1);
                const float tc = asm_ld1<S>(P.p, r1 + c0), td = asm_ld1<S>(P.p, r1 + c1);
                const float top = x.l0 * ta + x.l1 * tb;
                const float bot = x.l0 * tc + x.l1 * td;
                asm_push<T, V>(o, y.l0 * top + y.l1 * bot);
            }
        }
    }
}

__device__ __forceinline__ GruPart asm_scalar(const GruPart &v) {
    GruPart P;
    P.p = reinterpret_cast<const void *>(asm_s((long long)reinterpret_cast<uintptr_t>(v.p)));
    P.sn = asm_s(v.sn), P.sc = asm_s(v.sc), P.sh = asm_s(v.sh), P.sw = asm_s(v.sw);
    P.c0 = asm_s(v.c0), P.C = asm_s(v.C), P.mode = asm_s(v.mode), P.ek = asm_s(v.ek);
    P.SH = asm_s(v.SH), P.SW = asm_s(v.SW);
    P.scale_h = asm_s(v.scale_h), P.scale_w = asm_s(v.scale_w);
    return P;
}

// the source's element type is the outermost branch (uniform: P is in scalar
// registers), so each mode's loads are one straight-line block
template <class T, int V, bool INTER>
__device__ __forceinline__ void asm_unit(const GruPart &P, int n, int c, int h, int w, GruPack<T, V> &o) {
    if (P.ek == kF32) {
        if constexpr (V * sizeof(float) > 16) {
            // an fp32 source of a 16-bit dst: two halves of 16 source bytes, one after the other
            GruPack<T, V / 2> lo, hi;
            asm_unit_t<T, float, V / 2, INTER>(P, n, c, h, w, lo);
            __builtin_amdgcn_sched_barrier(0);
            asm_unit_t<T, float, V / 2, INTER>(P, n, INTER ? c + V / 2 : c, h, INTER ? w : w + V / 2, hi);
#pragma unroll
            for (int k = 0; k < V / 2; ++k) o.v[k] = lo.v[k], o.v[V / 2 + k] = hi.v[k];
        } else {
            asm_unit_t<T, float, V, INTER>(P, n, c, h, w, o);
        }
    }
    else if (P.ek == kF16) asm_unit_t<T, _Float16, V, INTER>(P, n, c, h, w, o);
    else asm_unit_t<T, __bf16, V, INTER>(P, n, c, h, w, o);
}

template <class T, int V, bool INTER>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8, 8))) void gru_assemble_kernel(GruAsmArgs a) {
    const uint32_t step = gridDim.x * 256u;
    for (uint32_t u = blockIdx.x * 256u + threadIdx.x; u < a.units; u += step) {
        const uint32_t outer = u / a.J, j = (u - outer * a.J) * V;
        int n, c, h, w;
        if constexpr (INTER) {        // outer: the pixel, j: the channel
            const uint32_t t = outer / (uint32_t)a.W;
            w = (int)(outer - t * (uint32_t)a.W);
            n = (int)(t / (uint32_t)a.H);
            h = (int)(t - (uint32_t)n * (uint32_t)a.H);
            c = (int)j;
        } else {                      // outer: the (n, c, h) row, j: the column
            const uint32_t t = outer / (uint32_t)a.H;
            h = (int)(outer - t * (uint32_t)a.H);
            n = (int)(t / (uint32_t)a.C);
            c = (int)(t - (uint32_t)n * (uint32_t)a.C);
            w = (int)j;
        }
        GruPack<T, V> o = {};
        // the unit's part, then one pass per part present in the wave with
        // that part's descriptor in scalar registers
        const int mine = (c >= a.cend[0]) + (c >= a.cend[1]) + (c >= a.cend[2]);
        for (bool todo = true; todo;) {
            const int p = __builtin_amdgcn_readfirstlane(mine);
            if (mine == p) {
                asm_unit<T, V, INTER>(asm_scalar(a.part[p]), n, c, h, w, o);
                todo = false;
            }
        }
        *reinterpret_cast<GruPack<T, V> *>(static_cast<T *>(a.dst) + (long long)n * a.dn + (long long)c * a.dc +
                                           (long long)h * a.dh + (long long)w * a.dw) = o;
    }
}

// Whether units of `bytes` bytes of dst (element size es) can be moved as one
// access each: dst and, where a unit reads them V-wide, the sources.
static bool asm_fits(const GruAsmArgs &a, int es, bool inter, int bytes) {
    const long long v = bytes / es;
    auto mult = [](long long size, long long stride, long long m) { return size <= 1 || stride % m == 0; };
    if (reinterpret_cast<uintptr_t>(a.dst) % (uintptr_t)bytes) return false;
    if (inter ? a.dc != 1 : (a.dw != 1 || a.W % v != 0)) return false;
    if (!mult(a.N, a.dn, v) || !mult(a.H, a.dh, v)) return false;
    if (inter ? !mult(a.W, a.dw, v) : !mult(a.C, a.dc, v)) return false;
    for (int i = 0; i < a.nparts; ++i) {
        const GruPart &P = a.part[i];
        const long long ses = P.ek == kF32 ? 4 : 2;
        const long long align = v * ses < 16 ? v * ses : 16, m = align / ses;
        const bool ptr_ok = reinterpret_cast<uintptr_t>(P.p) % (uintptr_t)align == 0;
        if (inter) {
            if (P.C % v != 0 || P.sc != 1 || !ptr_ok) return false;
            if (!mult(a.N, P.sn, m) || !mult(P.SH, P.sh, m) || !mult(P.SW, P.sw, m)) return false;
        } else if (P.mode == kPartCopy) {
            if (P.sw != 1 || !ptr_ok) return false;
            if (!mult(a.N, P.sn, m) || !mult(P.C, P.sc, m) || !mult(P.SH, P.sh, m)) return false;
        }
    }
    return true;
}

template <class T, int V, bool INTER>
static void asm_launch_v(GruAsmArgs &a, hipStream_t s) {
    const long long inner = (INTER ? a.C : a.W) / V;
    const long long units = (long long)a.N * a.H * (INTER ? a.W : a.C) * inner;
    a.J = (uint32_t)inner;
    a.units = (uint32_t)units;
    const long long cap = (long long)device_cus() * 8, need = (units + 255) / 256;
    hipLaunchKernelGGL((gru_assemble_kernel<T, V, INTER>), dim3((unsigned)(need < cap ? need : cap)), dim3(256), 0,
                       s, a);
}

template <class T, bool INTER>
static hipError_t asm_launch_t(GruAsmArgs &a, hipStream_t s) {
    constexpr int ES = (int)sizeof(T);
    if (asm_fits(a, ES, INTER, 16)) asm_launch_v<T, 16 / ES, INTER>(a, s);
    else if (asm_fits(a, ES, INTER, 8)) asm_launch_v<T, 8 / ES, INTER>(a, s);
    else asm_launch_v<T, 1, INTER>(a, s);
    return hipGetLastError();
}

}  // namespace rc

hipError_t rc_launch_gru_assemble(rc::GruAsmArgs &a, int ek, bool interleaved, hipStream_t s) {
    if ((long long)a.N * a.C * a.H * a.W <= 0) return hipSuccess;
    if (ek == rc::kF32)
        return interleaved ? rc::asm_launch_t<float, true>(a, s) : rc::asm_launch_t<float, false>(a, s);
    if (ek == rc::kF16)
        return interleaved ? rc::asm_launch_t<_Float16, true>(a, s) : rc::asm_launch_t<_Float16, false>(a, s);
    if (ek == rc::kBF16)
        return interleaved ? rc::asm_launch_t<__bf16, true>(a, s) : rc::asm_launch_t<__bf16, false>(a, s);
    return hipErrorInvalidValue;
}
