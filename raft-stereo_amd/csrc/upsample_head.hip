// The upsampling head of an inference forward (rc_upsample_head, gfx950): the
// convex upsampler of upsample.hip reading the mask as the update block's last
// convolution wrote it -- fp32, fp16 or bf16 logits, NCHW or channels-last,
// not yet scaled:
//     out[n][c][f h + i][f w + j] =
//         sum_k softmax_k(scale * mask[n][k f^2 + i f + j][h][w]) * f * flow[n][c][h + dy_k][w + dx_k]
// A logit is widened to fp32, multiplied by `scale` (one rounding, what
// `scale * mask.float()` stores) and from there goes through convex.h, the
// arithmetic of convex_upsample_kernel: the output equals rc_convex_upsample
// on that fp32 mask bit for bit, whatever the element type, layout class or
// access width.  The 0.25 * mask pass, the cast and the layout copy in front
// of rc_convex_upsample are three passes over the largest tensor of the tail
// that this kernel does not make.
//
// One workgroup of F waves per 64 consecutive lane groups, wave i taking
// sub-row i (the geometry of convex_upsample_bwd_kernel); there are no
// barriers and no LDS, the workgroup only keeps the F waves that share a
// pixel's logits and its flow neighbourhood on one CU at one time.
//
// Planar class (pixel stride 1, channel stride H W).  Wide: a lane owns the V
// consecutive pixels of 8 bytes (4 fp16 / bf16, 2 fp32) of the flattened (h, w)
// and each of its 9 F loads is one 8-byte vector, 512 contiguous bytes per
// wave; needs H W, the batch stride and the base to be multiples of 8 bytes.
// The raw vectors stay packed in registers and are widened one pixel at a
// time; f = 8 takes its eight sub-pixels in two passes of four, which keeps
// it free of scratch at the 256 registers a 512-lane workgroup leaves a lane.
// Narrow: V = 1, one element per load.
//
// Interleaved class (channel stride 1, pixel stride 9 F^2): the F logits
// k F^2 + i F .. + F - 1 of tap k are contiguous, and a lane (one pixel) loads
// them as one vector of F elements: 8 bytes at f = 4 in half precision, 16 at
// f = 4 in fp32 and at f = 8; the F waves of the workgroup together use every
// byte of the 64 pixels' contiguous 64 * 9 F^2 elements, so a line fetched for
// one wave is a cache hit for the others.  Staging that chunk through LDS was
// the alternative: it needs 72 KB at f = 8 in half precision (two workgroups
// per CU only just) and 144 KB in fp32, a barrier, and a padded row to keep
// the per-pixel reads off one bank; this variant needs none of it.  Narrow:
// F loads of one element, where the base or the batch stride is not a
// multiple of the vector.  The host picks the width (head_wide).
#include "convex.h"

namespace rc {

template <int EK> struct HeadElem { using T = uint16_t; };
template <> struct HeadElem<kF32> { using T = float; };

template <int EK>
__device__ __forceinline__ float head_widen(typename HeadElem<EK>::T v) {
    if constexpr (EK == kF32) return v;
    else if constexpr (EK == kF16) return f16_to_f32(v);
    else return bf16_to_f32(v);
}

template <class T, int V>
struct alignas(sizeof(T) * V < 16 ? sizeof(T) * V : 16) HeadPack {
    T v[V];
};

template <int EK, int F, bool INTER, bool WIDE>
__global__ __launch_bounds__(64 * F) void upsample_head_kernel(HeadArgs a) {
    using T = typename HeadElem<EK>::T;
    constexpr int V = (!INTER && WIDE) ? 8 / (int)sizeof(T) : 1;   // pixels per lane
    const int lane = threadIdx.x & 63, i = threadIdx.x >> 6;
    const long long g = (long long)blockIdx.x * 64 + lane;
    if (g >= a.groups) return;   // no barriers in this kernel
    const int H = a.H, W = a.W;
    const long long HW = (long long)H * W;
    const long long WO = (long long)W * F, per_img = (long long)H * F * WO;
    const long long p0 = g * V;   // V divides H W: the V pixels are of one image
    const long long n = p0 / HW, hw0 = p0 - n * HW;
    const T *m = static_cast<const T *>(a.mask) + n * a.msn;
    // Planar at f = 8: two passes of four sub-pixels j each, so the packed raw
    // logits of a pass (72 registers) and one pixel's weights fit beside each
    // other; everywhere else one pass of all F.
    constexpr int JB = (!INTER && F == 8) ? 4 : F;
#pragma unroll
    for (int jb = 0; jb < F; jb += JB) {
        // the pass's raw logits: raw[k] holds the F sub-pixels j of tap k
        // (interleaved), raw[k JB + j] the V pixels of (k, jb + j) (planar)
        HeadPack<T, INTER ? F : V> raw[INTER ? 9 : 9 * JB];
        if constexpr (INTER) {
            const T *q = m + hw0 * (9 * F * F) + i * F;
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                if constexpr (WIDE) {
                    raw[k] = *reinterpret_cast<const HeadPack<T, F> *>(q + k * F * F);
                } else {
#pragma unroll
                    for (int j = 0; j < F; ++j) raw[k].v[j] = q[k * F * F + j];
                }
            }
        } else {
            const T *q = m + (long long)(i * F + jb) * HW + hw0;
#pragma unroll
            for (int k = 0; k < 9; ++k)
#pragma unroll
                for (int j = 0; j < JB; ++j)
                    raw[k * JB + j] = *reinterpret_cast<const HeadPack<T, V> *>(q + ((long long)k * F * F + j) * HW);
        }
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const long long hw = hw0 + v;
            const int h = (int)(hw / W), w = (int)(hw - (long long)h * W);
            float wt[JB][9];
#pragma unroll
            for (int j = 0; j < JB; ++j) {
#pragma unroll
                for (int k = 0; k < 9; ++k) {
                    if constexpr (INTER) wt[j][k] = a.scale * head_widen<EK>(raw[k].v[j]);
                    else wt[j][k] = a.scale * head_widen<EK>(raw[k * JB + j].v[v]);
                }
                convex_weights(wt[j]);
            }
            for (int c = 0; c < a.C; ++c) {
                float nb[9];
                convex_neighbours<F>(a.flow + n * a.fsn + c * a.fsc, h, w, H, W, nb);
                float o[JB];
#pragma unroll
                for (int j = 0; j < JB; ++j) o[j] = convex_combine(wt[j], nb);
                store_row<JB>(a.out + (n * a.C + c) * per_img + (long long)(h * F + i) * WO + (long long)w * F + jb, o);
            }
        }
    }
}

// The widest access the mask's base, batch stride and plane size allow.
static bool head_wide(const HeadArgs &a, int es, int factor, bool inter) {
    const uintptr_t base = reinterpret_cast<uintptr_t>(a.mask);
    if (inter) {
        const long long bytes = factor * es < 16 ? factor * es : 16;
        return base % (uintptr_t)bytes == 0 && (a.msn * es) % bytes == 0;
    }
    const long long V = 8 / es;
    return base % 8 == 0 && a.msn % V == 0 && ((long long)a.H * a.W) % V == 0;
}

template <int EK, int F>
static void head_launch(const HeadArgs &a, bool inter, bool wide, unsigned nblk, hipStream_t s) {
    const dim3 grid(nblk), block(64 * F);
    if (inter) {
        if (wide) hipLaunchKernelGGL((upsample_head_kernel<EK, F, true, true>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((upsample_head_kernel<EK, F, true, false>), grid, block, 0, s, a);
    } else {
        if (wide) hipLaunchKernelGGL((upsample_head_kernel<EK, F, false, true>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((upsample_head_kernel<EK, F, false, false>), grid, block, 0, s, a);
    }
}

template <int EK>
static hipError_t head_factor(const HeadArgs &a, int factor, bool inter, bool wide, unsigned nblk, hipStream_t s) {
    switch (factor) {
        case 1: head_launch<EK, 1>(a, inter, wide, nblk, s); break;
        case 2: head_launch<EK, 2>(a, inter, wide, nblk, s); break;
        case 4: head_launch<EK, 4>(a, inter, wide, nblk, s); break;
        case 8: head_launch<EK, 8>(a, inter, wide, nblk, s); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace rc

hipError_t rc_launch_upsample_head(rc::HeadArgs &a, int ek, int factor, bool interleaved, hipStream_t s) {
    const long long pixels = (long long)a.N * a.H * a.W;
    if (pixels <= 0) return hipSuccess;
    const int es = ek == rc::kF32 ? 4 : 2;
    const bool wide = rc::head_wide(a, es, factor, interleaved);
    a.groups = (!interleaved && wide) ? pixels / (8 / es) : pixels;
    const long long nblk = (a.groups + 63) / 64;
    if (nblk > 0x7FFFFFFFLL) return hipErrorInvalidValue;
    switch (ek) {
        case rc::kF32: return rc::head_factor<rc::kF32>(a, factor, interleaved, wide, (unsigned)nblk, s);
        case rc::kF16: return rc::head_factor<rc::kF16>(a, factor, interleaved, wide, (unsigned)nblk, s);
        case rc::kBF16: return rc::head_factor<rc::kBF16>(a, factor, interleaved, wide, (unsigned)nblk, s);
        default: return hipErrorInvalidValue;
    }
}
