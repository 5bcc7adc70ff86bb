// What the convex upsampler's kernels share (upsample.hip: rc_convex_upsample,
// upsample_head.hip: rc_upsample_head): the softmax over the nine taps, the
// 3x3 neighbourhood of f * flow, the weighted sum and the store of a sub-row.
// Every kernel that goes through these computes the same bits from the same
// fp32 logits.
#pragma once
#include "common.h"

namespace rc {

// Nine fp32 logits -> their softmax weights, in place: max, expf, sum in
// ascending k, one reciprocal, nine products.
__device__ __forceinline__ void convex_weights(float (&wt)[9]) {
    float mx = -INFINITY;
#pragma unroll
    for (int k = 0; k < 9; ++k) mx = fmaxf(mx, wt[k]);
    float sum = 0.0f;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        wt[k] = expf(wt[k] - mx);
        sum += wt[k];
    }
    const float inv = 1.0f / sum;
#pragma unroll
    for (int k = 0; k < 9; ++k) wt[k] *= inv;
}

// nb[k] = f * fl[h + dy_k][w + dx_k], k = 3 (dy + 1) + (dx + 1), zeros outside
// the H x W image; fl: one channel, rows of W unit-stride elements.
template <int F>
__device__ __forceinline__ void convex_neighbours(const float *fl, int h, int w, int H, int W, float (&nb)[9]) {
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const int yy = h + k / 3 - 1, xx = w + k % 3 - 1;
        nb[k] = (yy >= 0 && yy < H && xx >= 0 && xx < W) ? (float)F * fl[(long long)yy * W + xx] : 0.0f;
    }
}

// sum_k wt[k] * nb[k]: the fmaf chain in ascending k from 0.
__device__ __forceinline__ float convex_combine(const float (&wt)[9], const float (&nb)[9]) {
    float acc = 0.0f;
#pragma unroll
    for (int k = 0; k < 9; ++k) acc = fmaf(wt[k], nb[k], acc);
    return acc;
}

// the f outputs of a sub-row as one vector store (dst aligned to min(16, 4 f) bytes)
template <int F>
__device__ __forceinline__ void store_row(float *dst, const float (&v)[F]) {
    if constexpr (F == 4) {
        *reinterpret_cast<f32x4 *>(dst) = f32x4{v[0], v[1], v[2], v[3]};
    } else if constexpr (F == 8) {
        *reinterpret_cast<f32x4 *>(dst) = f32x4{v[0], v[1], v[2], v[3]};
        *reinterpret_cast<f32x4 *>(dst + 4) = f32x4{v[4], v[5], v[6], v[7]};
    } else if constexpr (F == 2) {
        *reinterpret_cast<f32x2 *>(dst) = f32x2{v[0], v[1]};
    } else {
        dst[0] = v[0];
    }
}

}  // namespace rc
