// Convex upsampling of the low-resolution flow (gfx950), SURVEY.md §8f rank 3.
//
// The reference's update block already produces the upsampling mask
// (model.py:238-241, scaled by 0.25 at :264): (f^2)*9 channels per
// low-resolution pixel, f = 2^n_downsample (:236).  Its truncated forward
// never consumes it.  RAFT-Stereo's convex upsampler
// turns the mask into softmax weights over the 3x3 neighbourhood of every
// low-resolution pixel and combines f * flow there:
//     up[n][c][f h + i][f w + j] =
//         sum_k softmax_k(mask[n][k f^2 + i f + j][h][w]) * f * flow[n][c][h + dy_k][w + dx_k]
// with k = 3 (dy + 1) + (dx + 1) (F.unfold's row-major 3x3 order) and zeros
// outside the image.  Parity is checked against oracle/torch_ref.py's
// restatement (F.unfold + softmax); the reference has no upsampler to pin it.
//
// One lane per (n, h, i, w): the f outputs of sub-row i of low-resolution
// pixel (h, w).  Consecutive lanes take consecutive w, so each of the 9 f
// mask loads of a lane is part of one contiguous 256-B wave access, every
// mask element is read once, and the f outputs go out as one vector store
// (f = 4: 16 B per lane, 1 KB per wave).  The 3x3 flow neighbourhood is
// loaded once per lane.  HBM-bound: 4 (9 f^2 + C + f^2 C) bytes per
// low-resolution pixel.
//
// Backward (rc_convex_upsample_backward): nothing is saved
// from the forward but its inputs.  convex_upsample_bwd_kernel<F> runs one
// workgroup of F waves per 64 consecutive low-resolution pixels, wave i
// taking sub-row i (the forward's lane: same mask addresses, and the F
// grad_out values of a channel come in as one vector, the mirror of
// store_row).  Each lane recomputes its softmax weights in the forward's
// arithmetic and, with g = grad_out and nb = f * flow around the pixel,
//     d[j][k]          = sum_c g[c][j] * nb[c][k]
//     grad_mask[j][k]  = wt[j][k] * (d[j][k] - sum_k' wt[j][k'] d[j][k'])
//     P_i[c][k]        = f * sum_j wt[j][k] * g[c][j]
// grad_mask goes out at the addresses the mask came from.  The F sub-row
// partials P_i of a pixel meet in LDS and are summed in ascending i into the
// workspace P[n][c][k][h][w]; convex_upsample_bwd_gather_kernel then sums the
// nine taps grad_flow[n][c][y][x] = sum_k P[n][c][k][y - dy_k][x - dx_k] in
// ascending k.  No atomics anywhere: pixel p owns row p, every sum has a fixed
// order, and repeated runs agree bit for bit.  Every mask and grad_out
// element is read once and every grad_mask element written once:
// 4 (9 f^2 + f^2 C + C) bytes read and 4 (9 f^2 + C) written per
// low-resolution pixel, plus 4 * 9 C each way through the workspace.
#include "convex.h"

namespace rc {

template <int F>
__global__ __launch_bounds__(256) void convex_upsample_kernel(const float *__restrict__ flow,
                                                              const float *__restrict__ mask,
                                                              float *__restrict__ out, int N, int C,
                                                              int H, int W, long long total) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;   // no barriers in this kernel
    const int w = (int)(idx % W);
    long long t = idx / W;
    const int i = (int)(t % F);
    t /= F;
    const int h = (int)(t % H);
    const int n = (int)(t / H);
    const long long HW = (long long)H * W;
    const long long WO = (long long)W * F, per_img = (long long)H * F * WO;
    const float *m = mask + ((long long)n * 9 * F * F + i * F) * HW + (long long)h * W + w;
    // softmax weights of the f sub-pixels (i, j), j = 0..f-1
    float wt[F][9];
#pragma unroll
    for (int j = 0; j < F; ++j) {
#pragma unroll
        for (int k = 0; k < 9; ++k) wt[j][k] = m[((long long)k * F * F + j) * HW];
        convex_weights(wt[j]);
    }
    for (int c = 0; c < C; ++c) {
        float nb[9];
        convex_neighbours<F>(flow + ((long long)n * C + c) * HW, h, w, H, W, nb);
        float o[F];
#pragma unroll
        for (int j = 0; j < F; ++j) o[j] = convex_combine(wt[j], nb);
        store_row<F>(out + ((long long)n * C + c) * per_img + (long long)(h * F + i) * WO + (long long)w * F, o);
    }
}

template <int F>
__device__ __forceinline__ void load_row(const float *src, float (&v)[F]) {
    if constexpr (F == 4) {
        const f32x4 a = *reinterpret_cast<const f32x4 *>(src);
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
    } else if constexpr (F == 8) {
        const f32x4 a = *reinterpret_cast<const f32x4 *>(src);
        const f32x4 b = *reinterpret_cast<const f32x4 *>(src + 4);
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
        v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    } else if constexpr (F == 2) {
        const f32x2 a = *reinterpret_cast<const f32x2 *>(src);
        v[0] = a.x; v[1] = a.y;
    } else {
        v[0] = src[0];
    }
}

// Workgroup = F waves over the 64 consecutive pixels p0 .. p0 + 63 of the
// flattened (n, h, w); wave i = sub-row i.  gmask == nullptr skips grad_mask,
// ws == nullptr skips the partial sums (both are kernel arguments, so every
// branch around a barrier is workgroup-uniform).  Lanes past the last pixel
// stay in the kernel for the barriers and touch no global memory.
template <int F>
__global__ __launch_bounds__(64 * F) void convex_upsample_bwd_kernel(
    const float *__restrict__ flow, const float *__restrict__ mask, const float *__restrict__ gout,
    float *__restrict__ gmask, float *__restrict__ ws, int C, int H, int W, long long total) {
    __shared__ float part[F][9][64];
    const int lane = threadIdx.x & 63, i = threadIdx.x >> 6;
    const long long p0 = (long long)blockIdx.x * 64;
    const long long p = p0 + lane;
    const bool valid = p < total;
    const long long HW = (long long)H * W;
    const long long WO = (long long)W * F, per_img = (long long)H * F * WO;
    const long long pc = valid ? p : total - 1;   // clamped: index arithmetic only
    const long long n = pc / HW;
    const long long hw = pc - n * HW;
    const int h = (int)(hw / W), w = (int)(hw - (long long)h * W);
    const long long moff = (n * 9 * F * F + i * F) * HW + hw;
    // softmax weights of the f sub-pixels (i, j): the forward's arithmetic
    float wt[F][9];
#pragma unroll
    for (int j = 0; j < F; ++j) {
        float mx = -INFINITY;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            wt[j][k] = valid ? mask[moff + ((long long)k * F * F + j) * HW] : 0.0f;
            mx = fmaxf(mx, wt[j][k]);
        }
        float sum = 0.0f;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            wt[j][k] = expf(wt[j][k] - mx);
            sum += wt[j][k];
        }
        const float inv = 1.0f / sum;
#pragma unroll
        for (int k = 0; k < 9; ++k) wt[j][k] *= inv;
    }
    float d[F][9];
#pragma unroll
    for (int j = 0; j < F; ++j)
#pragma unroll
        for (int k = 0; k < 9; ++k) d[j][k] = 0.0f;
    for (int c = 0; c < C; ++c) {
        float g[F];
#pragma unroll
        for (int j = 0; j < F; ++j) g[j] = 0.0f;
        if (valid)
            load_row<F>(gout + (n * C + c) * per_img + (long long)(h * F + i) * WO + (long long)w * F, g);
        if (gmask) {
            const float *fl = flow + (n * C + c) * HW;
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                const int yy = h + k / 3 - 1, xx = w + k % 3 - 1;
                const float nb = (valid && yy >= 0 && yy < H && xx >= 0 && xx < W)
                                     ? (float)F * fl[(long long)yy * W + xx] : 0.0f;
#pragma unroll
                for (int j = 0; j < F; ++j) d[j][k] = fmaf(g[j], nb, d[j][k]);
            }
        }
        if (ws) {
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                float acc = 0.0f;
#pragma unroll
                for (int j = 0; j < F; ++j) acc = fmaf(wt[j][k], g[j], acc);
                part[i][k][lane] = (float)F * acc;
            }
            __syncthreads();
            // the F sub-rows of a pixel, in ascending i; tap plane k of the
            // workspace is written 64 consecutive pixels at a time
            for (int o = threadIdx.x; o < 9 * 64; o += 64 * F) {
                const int k = o >> 6, l = o & 63;
                float acc = part[0][k][l];
#pragma unroll
                for (int r = 1; r < F; ++r) acc += part[r][k][l];
                const long long q = p0 + l;
                if (q < total) {
                    const long long qn = q / HW;
                    ws[((qn * C + c) * 9 + k) * HW + (q - qn * HW)] = acc;
                }
            }
            __syncthreads();   // part is rewritten for the next channel
        }
    }
    if (gmask && valid) {
#pragma unroll
        for (int j = 0; j < F; ++j) {
            float s = 0.0f;
#pragma unroll
            for (int k = 0; k < 9; ++k) s = fmaf(wt[j][k], d[j][k], s);
#pragma unroll
            for (int k = 0; k < 9; ++k)
                gmask[moff + ((long long)k * F * F + j) * HW] = wt[j][k] * (d[j][k] - s);
        }
    }
}

// grad_flow[n][c][y][x] = sum_k P[n][c][k][y - dy_k][x - dx_k], ascending k,
// taps whose source pixel lies outside the image dropped.  One lane per
// grad_flow element; each of the nine reads is coalesced along x.
__global__ __launch_bounds__(256) void convex_upsample_bwd_gather_kernel(
    const float *__restrict__ ws, float *__restrict__ gflow, int H, int W, long long total) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;   // no barriers in this kernel
    const long long HW = (long long)H * W;
    const long long nc = idx / HW;
    const long long yx = idx - nc * HW;
    const int y = (int)(yx / W), x = (int)(yx - (long long)y * W);
    const float *P = ws + nc * 9 * HW;
    float acc = 0.0f;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const int yy = y - (k / 3 - 1), xx = x - (k % 3 - 1);
        if (yy >= 0 && yy < H && xx >= 0 && xx < W) acc += P[(long long)k * HW + (long long)yy * W + xx];
    }
    gflow[idx] = acc;
}

}  // namespace rc

hipError_t rc_launch_convex_upsample(const float *flow, const float *mask, int N, int C, int H,
                                     int W, int factor, float *out, hipStream_t s) {
    const long long total = (long long)N * H * W * factor;   // lanes: (n, h, i, w)
    if (total <= 0) return hipSuccess;
    const unsigned nblk = (unsigned)((total + 255) / 256);
    switch (factor) {
        case 1: hipLaunchKernelGGL(rc::convex_upsample_kernel<1>, dim3(nblk), dim3(256), 0, s, flow, mask, out, N, C, H, W, total); break;
        case 2: hipLaunchKernelGGL(rc::convex_upsample_kernel<2>, dim3(nblk), dim3(256), 0, s, flow, mask, out, N, C, H, W, total); break;
        case 4: hipLaunchKernelGGL(rc::convex_upsample_kernel<4>, dim3(nblk), dim3(256), 0, s, flow, mask, out, N, C, H, W, total); break;
        case 8: hipLaunchKernelGGL(rc::convex_upsample_kernel<8>, dim3(nblk), dim3(256), 0, s, flow, mask, out, N, C, H, W, total); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t rc_launch_convex_upsample_bwd(const float *flow, const float *mask, const float *grad_out,
                                         int N, int C, int H, int W, int factor, float *grad_flow,
                                         float *grad_mask, float *workspace, hipStream_t s) {
    const long long total = (long long)N * H * W;   // low-resolution pixels
    if (total <= 0) return hipSuccess;
    float *ws = grad_flow ? workspace : nullptr;
    const unsigned nblk = (unsigned)((total + 63) / 64);
    switch (factor) {
        case 1: hipLaunchKernelGGL(rc::convex_upsample_bwd_kernel<1>, dim3(nblk), dim3(64), 0, s, flow, mask, grad_out, grad_mask, ws, C, H, W, total); break;
        case 2: hipLaunchKernelGGL(rc::convex_upsample_bwd_kernel<2>, dim3(nblk), dim3(128), 0, s, flow, mask, grad_out, grad_mask, ws, C, H, W, total); break;
        case 4: hipLaunchKernelGGL(rc::convex_upsample_bwd_kernel<4>, dim3(nblk), dim3(256), 0, s, flow, mask, grad_out, grad_mask, ws, C, H, W, total); break;
        case 8: hipLaunchKernelGGL(rc::convex_upsample_bwd_kernel<8>, dim3(nblk), dim3(512), 0, s, flow, mask, grad_out, grad_mask, ws, C, H, W, total); break;
        default: return hipErrorInvalidValue;
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !grad_flow) return e;
    const long long nel = total * C;
    hipLaunchKernelGGL(rc::convex_upsample_bwd_gather_kernel, dim3((unsigned)((nel + 255) / 256)), dim3(256), 0, s,
                       (const float *)ws, grad_flow, H, W, nel);
    return hipGetLastError();
}
