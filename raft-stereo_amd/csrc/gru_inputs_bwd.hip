// The adjoint of the ConvGRU input assembly (gru_inputs.hip): from the gradient
// G of the assembled N x sum(C) x H x W buffer, the gradient of every part's
// source, one memory-bound launch (rc_gru_assemble_backward; gfx950).
//
// G = g, or g + g2 from channel g2_c0 on (added in fp32 after widening): the
// training route hands the gradients of [h, x] and of [r*h, x] to one launch
// instead of adding them per part.  g2 is never read below g2_c0: where it
// does not count, its load goes to g's address and a select drops the value.
//
// G is planar or interleaved.  A work unit is V elements of ONE OUTPUT along
// the unit-stride axis of G's layout class, stored as one access (two for an
// fp32 output of a 16-bit G): V channels of one source pixel (interleaved) or
// V columns of one source row of one channel (planar); 16 bytes of G's
// element type where every base, stride and length allows, else 8, else one
// element, which also serves outputs of the other class (asmb_fits chooses).
// The unit index runs over the concatenated outputs; a wave finds its part
// from the cumulative unit ends and takes the parts present in it one after
// the other (a uniform loop over the parts), each descriptor in scalar
// registers.  Every lane owns what it
// stores: no atomics, every sum in a fixed order, so the results repeat bit
// for bit and are the same for every layout and width.  An interleaved unit
// loads G V-wide per tap; a planar one loads a copied part V-wide and gathers
// the others element by element in a rolled loop (asmb_push), as the forward.
//
// Arithmetic: fp32 on the widened inputs, each operation rounded on its own
// (-ffp-contract=off), one rounding at the store (out_cvt).
//   copy      grad = (S)G.
//   pool2x    source pixel (y, x) lies in the windows oy = y / 2 (y even) or
//             (y - 1) / 2 and (y + 1) / 2 (y odd; only oy < H), likewise along
//             W: the sum of their G, row-major from 0.0f (a window that does
//             not count adds 0.0f, its load goes to a clamped address), then
//             / 9.0f, correctly rounded.
//   bilinear  per axis the weight of destination d on source s is
//             (i0(d) == s ? l0(d) : 0) + (i1(d) == s ? l1(d) : 0) with the
//             forward's asm_axis;  acc = sum_dy wy(dy) * (sum_dx wx(dx) *
//             G[dy][dx]), both ascending from 0.0f.  The destinations that
//             reach s are those with i0(d) in {s - 1, s}: i0 is monotone in d
//             (the fp32 multiply is), so two binary searches on i0 bound
//             them and the scale is never inverted.  The loops are run-time
//             loops: a downscale has ranges of 0 to 2, S == 1 or D == 1 the
//             whole axis.  A source pixel nothing reads gets +0.
#include "gru_inputs.h"  // asm_ld1, asm_ldv, asm_axis, asm_clamp, asm_trips, asm_s

namespace rc {

// Where to read G for one unit: g, and g2 where it counts (else g again).
struct AsmbG {
    const void *g, *p2;
    bool two;
};

template <class T>
__device__ __forceinline__ float asmb_g1(const AsmbG &q, long long off) {
    const float a = asm_ld1<T>(q.g, off), b = asm_ld1<T>(q.p2, off);
    return q.two ? a + b : a;
}

template <class T, int V>
__device__ __forceinline__ void asmb_gv(const AsmbG &q, long long off, float (&G)[V]) {
    const GruPack<T, V> a = asm_ldv<T, V>(q.g, off), b = asm_ldv<T, V>(q.p2, off);
#pragma unroll
    for (int k = 0; k < V; ++k) {
        const float fa = (float)a.v[k];
        G[k] = q.two ? fa + (float)b.v[k] : fa;
    }
}

// V results as accesses of at most 16 bytes of the output's type S
template <class S, int V>
__device__ __forceinline__ void asmb_store(void *p, long long off, const float (&r)[V]) {
    constexpr int M = sizeof(S) * V > 16 ? 16 / (int)sizeof(S) : V;
#pragma unroll
    for (int q = 0; q < V; q += M) {
        GruPack<S, M> o;
#pragma unroll
        for (int k = 0; k < M; ++k) o.v[k] = out_cvt<S>(r[q + k]);
        *reinterpret_cast<GruPack<S, M> *>(static_cast<S *>(p) + off + q) = o;
    }
}

// r as a shift register (asm_push of the forward, on the fp32 results)
template <int V>
__device__ __forceinline__ void asmb_push(float (&r)[V], float v) {
#pragma unroll
    for (int k = 0; k + 1 < V; ++k) r[k] = r[k + 1];
    asm("" : "+v"(v));
    r[V - 1] = v;
}

// The first d of [0, D] with asm_axis(scale, d, S).i0 >= t (D: there is none)
__device__ __forceinline__ int asmb_first(float scale, int S, int D, int t) {
    int lo = 0, hi = D;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (asm_axis(scale, mid, S).i0 >= t) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

__device__ __forceinline__ float asmb_weight(const AsmAxis &x, int s) {
    return (x.i0 == s ? x.l0 : 0.0f) + (x.i1 == s ? x.l1 : 0.0f);
}

// The two windows of source index i along an axis pooled to D
struct AsmbWin {
    int o0, o1;     // o1 clamped into the axis
    bool ok1;
};
__device__ __forceinline__ AsmbWin asmb_win(int i, int D) {
    AsmbWin w;
    w.o0 = i >> 1;
    const int o1 = (i + 1) >> 1;
    w.ok1 = (i & 1) != 0 && o1 < D;
    w.o1 = o1 < D ? o1 : D - 1;
    return w;
}

// One unit of part P, whose output holds elements of type S: unit lu of the
// part.  Interleaved: channels c .. c+V-1 of source pixel (y, x); planar:
// columns x .. x+V-1 of row y of channel c.
template <class T, class S, int V, bool INTER>
__device__ __forceinline__ void asmb_unit_t(const GruAsmBwdArgs &a, const GruBwdPart &P, uint32_t lu) {
    const uint32_t outer = lu / P.J, j = (lu - outer * P.J) * V;
    int n, c, y, x;
    if constexpr (INTER) {        // outer: the source pixel, j: the channel
        const uint32_t t = outer / (uint32_t)P.SW;
        x = (int)(outer - t * (uint32_t)P.SW);
        n = (int)(t / (uint32_t)P.SH);
        y = (int)(t - (uint32_t)n * (uint32_t)P.SH);
        c = (int)j;
    } else {                      // outer: the (n, c, y) row, j: the column
        const uint32_t t = outer / (uint32_t)P.SH;
        y = (int)(outer - t * (uint32_t)P.SH);
        n = (int)(t / (uint32_t)P.C);
        c = (int)(t - (uint32_t)n * (uint32_t)P.C);
        x = (int)j;
    }
    const int cg = P.c0 + c;
    AsmbG q;
    q.two = a.g2 != nullptr && cg >= a.g2_c0;
    q.g = a.g, q.p2 = q.two ? a.g2 : a.g;
    const long long b = (long long)n * a.gn + (long long)cg * a.gc;
    float r[V];
    if (P.mode == kPartCopy) {
        asmb_gv<T, V>(q, b + (long long)y * a.gh + (long long)x * a.gw, r);
    } else if (P.mode == kPartPool2x) {
        const AsmbWin wy = asmb_win(y, a.H);
        const long long r0 = b + (long long)wy.o0 * a.gh, r1 = b + (long long)wy.o1 * a.gh;
        if constexpr (INTER) {
            const AsmbWin wx = asmb_win(x, a.W);
            const long long c0 = (long long)wx.o0 * a.gw, c1 = (long long)wx.o1 * a.gw;
            float t0[V], t1[V];
            asmb_gv<T, V>(q, r0 + c0, t0);
            asmb_gv<T, V>(q, r0 + c1, t1);
#pragma unroll
            for (int k = 0; k < V; ++k) r[k] = (0.0f + t0[k]) + (wx.ok1 ? t1[k] : 0.0f);
            asmb_gv<T, V>(q, r1 + c0, t0);
            asmb_gv<T, V>(q, r1 + c1, t1);
#pragma unroll
            for (int k = 0; k < V; ++k) {
                r[k] = r[k] + (wy.ok1 ? t0[k] : 0.0f);
                r[k] = r[k] + (wy.ok1 && wx.ok1 ? t1[k] : 0.0f);
                r[k] = r[k] / 9.0f;
            }
        } else {
#pragma unroll 1
            for (int k = 0, trips = asm_trips<V>(); k < trips; ++k) {
                const AsmbWin wx = asmb_win(x + k, a.W);
                const long long c0 = (long long)wx.o0 * a.gw, c1 = (long long)wx.o1 * a.gw;
                const float t00 = asmb_g1<T>(q, r0 + c0), t01 = asmb_g1<T>(q, r0 + c1);
                const float t10 = asmb_g1<T>(q, r1 + c0), t11 = asmb_g1<T>(q, r1 + c1);
                float acc = (0.0f + t00) + (wx.ok1 ? t01 : 0.0f);
                acc = acc + (wy.ok1 ? t10 : 0.0f);
                acc = acc + (wy.ok1 && wx.ok1 ? t11 : 0.0f);
                asmb_push<V>(r, acc / 9.0f);
            }
        }
    } else {
        const int ylo = asmb_first(P.scale_h, P.SH, a.H, y - 1), yhi = asmb_first(P.scale_h, P.SH, a.H, y + 1);
        if constexpr (INTER) {
            const int xlo = asmb_first(P.scale_w, P.SW, a.W, x - 1), xhi = asmb_first(P.scale_w, P.SW, a.W, x + 1);
#pragma unroll
            for (int k = 0; k < V; ++k) r[k] = 0.0f;
#pragma unroll 1
            for (int dy = ylo; dy < yhi; ++dy) {
                const float wy = asmb_weight(asm_axis(P.scale_h, dy, P.SH), y);
                const long long row = b + (long long)dy * a.gh;
                float inner[V];
#pragma unroll
                for (int k = 0; k < V; ++k) inner[k] = 0.0f;
#pragma unroll 1
                for (int dx = xlo; dx < xhi; ++dx) {
                    const float wx = asmb_weight(asm_axis(P.scale_w, dx, P.SW), x);
                    float G[V];
                    asmb_gv<T, V>(q, row + (long long)dx * a.gw, G);
#pragma unroll
                    for (int k = 0; k < V; ++k) inner[k] = inner[k] + wx * G[k];
                }
#pragma unroll
                for (int k = 0; k < V; ++k) r[k] = r[k] + wy * inner[k];
            }
        } else {
#pragma unroll 1
            for (int k = 0, trips = asm_trips<V>(); k < trips; ++k) {
                const int xs = x + k;
                const int xlo = asmb_first(P.scale_w, P.SW, a.W, xs - 1), xhi = asmb_first(P.scale_w, P.SW, a.W, xs + 1);
                float acc = 0.0f;
#pragma unroll 1
                for (int dy = ylo; dy < yhi; ++dy) {
                    const float wy = asmb_weight(asm_axis(P.scale_h, dy, P.SH), y);
                    const long long row = b + (long long)dy * a.gh;
                    float inner = 0.0f;
#pragma unroll 1
                    for (int dx = xlo; dx < xhi; ++dx) {
                        const float wx = asmb_weight(asm_axis(P.scale_w, dx, P.SW), xs);
                        inner = inner + wx * asmb_g1<T>(q, row + (long long)dx * a.gw);
                    }
                    acc = acc + wy * inner;
                }
                asmb_push<V>(r, acc);
            }
        }
    }
    asmb_store<S, V>(P.p, (long long)n * P.sn + (long long)c * P.sc + (long long)y * P.sh + (long long)x * P.sw, r);
}

__device__ __forceinline__ GruBwdPart asmb_scalar(const GruBwdPart &v) {
    GruBwdPart P;
    P.p = reinterpret_cast<void *>(asm_s((long long)reinterpret_cast<uintptr_t>(v.p)));
    P.sn = asm_s(v.sn), P.sc = asm_s(v.sc), P.sh = asm_s(v.sh), P.sw = asm_s(v.sw);
    P.c0 = asm_s(v.c0), P.C = asm_s(v.C), P.mode = asm_s(v.mode), P.ek = asm_s(v.ek);
    P.SH = asm_s(v.SH), P.SW = asm_s(v.SW);
    P.scale_h = asm_s(v.scale_h), P.scale_w = asm_s(v.scale_w);
    P.J = (uint32_t)asm_s((int)v.J);
    P.u0 = (unsigned long long)asm_s((long long)v.u0);
    return P;
}

template <class T, int V, bool INTER>
__global__ __launch_bounds__(256) void gru_assemble_bwd_kernel(GruAsmBwdArgs a) {
    const unsigned long long step = (unsigned long long)gridDim.x * 256u;
    for (unsigned long long u = blockIdx.x * 256u + threadIdx.x; u < a.units; u += step) {
        // the unit's part, then one pass per part present in the wave with
        // that part's descriptor in scalar registers; the output's element
        // type is the outermost branch (uniform).  The passes are a uniform
        // loop over the parts, which a wave without a unit of the part skips:
        // the forward's loop on readfirstlane(mine) does not survive here (to
        // the compiler readfirstlane is a pure function of its operand; it
        // sank the body out of the loop, where the whole wave ran it with the
        // first lane's descriptor).
        const int mine = (u >= a.uend[0]) + (u >= a.uend[1]) + (u >= a.uend[2]);
#pragma unroll 1
        for (int p = 0; p < a.nparts; ++p) {
            if (mine != p) continue;
            const GruBwdPart P = asmb_scalar(a.part[p]);
            const uint32_t lu = (uint32_t)(u - P.u0);
            if (P.ek == kF32) asmb_unit_t<T, float, V, INTER>(a, P, lu);
            else if (P.ek == kF16) asmb_unit_t<T, _Float16, V, INTER>(a, P, lu);
            else asmb_unit_t<T, __bf16, V, INTER>(a, P, lu);
        }
    }
}

// Whether units of `bytes` bytes of G's element type (size es) can be moved
// as one access each: G where a unit reads it V-wide, and every output.
static bool asmb_fits(const GruAsmBwdArgs &a, int es, bool inter, int bytes) {
    const long long v = bytes / es;
    auto mult = [](long long size, long long stride, long long m) { return size <= 1 || stride % m == 0; };
    if (reinterpret_cast<uintptr_t>(a.g) % (uintptr_t)bytes) return false;
    if (a.g2 && reinterpret_cast<uintptr_t>(a.g2) % (uintptr_t)bytes) return false;
    if (inter ? a.gc != 1 : a.gw != 1) return false;
    if (!mult(a.N, a.gn, v) || !mult(a.H, a.gh, v)) return false;
    if (inter ? !mult(a.W, a.gw, v) : !mult(a.C, a.gc, v)) return false;
    if (inter && a.g2 && a.g2_c0 % v != 0) return false;       // a unit is on one side of g2_c0
    for (int i = 0; i < a.nparts; ++i) {
        const GruBwdPart &P = a.part[i];
        if (!P.p) continue;
        const long long ses = P.ek == kF32 ? 4 : 2;
        const long long align = v * ses < 16 ? v * ses : 16, m = align / ses;
        if (reinterpret_cast<uintptr_t>(P.p) % (uintptr_t)align) return false;
        if (inter) {
            if (P.C % v != 0 || P.c0 % v != 0 || P.sc != 1) return false;
            if (!mult(a.N, P.sn, m) || !mult(P.SH, P.sh, m) || !mult(P.SW, P.sw, m)) return false;
        } else {
            if (P.SW % v != 0 || P.sw != 1) return false;
            if (!mult(a.N, P.sn, m) || !mult(P.C, P.sc, m) || !mult(P.SH, P.sh, m)) return false;
        }
    }
    return true;
}

template <class T, int V, bool INTER>
static void asmb_launch_v(GruAsmBwdArgs &a, hipStream_t s) {
    unsigned long long u = 0;
    for (int i = 0; i < kGruMaxParts; ++i) {
        GruBwdPart &P = a.part[i];
        P.u0 = u;
        P.J = 1;
        if (i < a.nparts && P.p) {
            P.J = (uint32_t)((INTER ? P.C : P.SW) / V);
            u += (unsigned long long)a.N * P.SH * (INTER ? P.SW : P.C) * P.J;
        }
        a.uend[i] = u;
    }
    a.units = u;
    const unsigned long long cap = (unsigned long long)device_cus() * 8, need = (u + 255) / 256;
    hipLaunchKernelGGL((gru_assemble_bwd_kernel<T, V, INTER>), dim3((unsigned)(need < cap ? need : cap)), dim3(256), 0,
                       s, a);
}

template <class T, bool INTER>
static hipError_t asmb_launch_t(GruAsmBwdArgs &a, hipStream_t s) {
    constexpr int ES = (int)sizeof(T);
    if (asmb_fits(a, ES, INTER, 16)) asmb_launch_v<T, 16 / ES, INTER>(a, s);
    else if (asmb_fits(a, ES, INTER, 8)) asmb_launch_v<T, 8 / ES, INTER>(a, s);
    else asmb_launch_v<T, 1, INTER>(a, s);
    return hipGetLastError();
}

}  // namespace rc

hipError_t rc_launch_gru_assemble_bwd(rc::GruAsmBwdArgs &a, int ek, bool interleaved, hipStream_t s) {
    if ((long long)a.N * a.C * a.H * a.W <= 0) return hipSuccess;
    if (ek == rc::kF32)
        return interleaved ? rc::asmb_launch_t<float, true>(a, s) : rc::asmb_launch_t<float, false>(a, s);
    if (ek == rc::kF16)
        return interleaved ? rc::asmb_launch_t<_Float16, true>(a, s) : rc::asmb_launch_t<_Float16, false>(a, s);
    if (ek == rc::kBF16)
        return interleaved ? rc::asmb_launch_t<__bf16, true>(a, s) : rc::asmb_launch_t<__bf16, false>(a, s);
    return hipErrorInvalidValue;
}
