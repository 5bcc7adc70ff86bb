// The backward of the ConvGRU glue kernels (gru_gates.hip), for training with
// the fused update block (rc_gru_gates_backward, rc_gru_blend_backward; gfx950):
//   blend:  q      = tanh(q_pre + cq)
//           g_z    = g_out * (q - h)
//           g_qpre = (g_out * z) * (1 - q*q)         also the gradient of cq
//           g_h    = g_out * (1 - z)
//   gates:  r      = sigmoid(r_pre + cr)
//           g_zpre = g_z * ((1 - z) * z)             also the gradient of cz
//           g_rpre = (g_rh * h) * ((1 - r) * r)      also the gradient of cr
//           g_h    = g_rh * r
// r and q are recomputed from the pre-activations with the forward's own
// gru_sigmoid and tanhf, so they are the forward's values bit for bit and
// nothing but z is kept from the forward.  At saturation (r = 0 or 1, q = +-1)
// the factor (1 - r) * r or 1 - q*q is exactly 0, as PyTorch's
// sigmoid_backward / tanh_backward give it.
//
// Operands, access widths, the loop and the arithmetic rules are the forward
// kernels' (gru_gates.h, and the header comment of gru_gates.hip): fp32 on the
// widened inputs, each operation rounded on its own in the order written
// above, one rounding to T at the store.
// Aliasing: a unit reads all its inputs before it writes, and no other unit
// touches its elements, so an output may be an input (same address and
// strides); two outputs must not be the same array.
#include "gru_gates.h"

namespace rc {

// operands: 0 g_z, 1 g_rh, 2 z, 3 r_pre, 4 cr, 5 h, 6 g_zpre, 7 g_rpre, 8 g_h
template <class T, int V>
__global__ __launch_bounds__(256) void gru_gates_bwd_kernel(GruBwdArgs a) {
    const uint32_t step = gridDim.x * 256u;
    for (uint32_t u = blockIdx.x * 256u + threadIdx.x; u < a.units; u += step) {
        const uint32_t row = u / a.J, j = u - row * a.J;
        const uint32_t n = row / a.O, o = row - n * a.O;
        const long long i = (long long)j * V;
        const GruPack<T, V> gz = gru_load<T, V>(a.op[0], n, o, i), grh = gru_load<T, V>(a.op[1], n, o, i);
        const GruPack<T, V> z = gru_load<T, V>(a.op[2], n, o, i), rp = gru_load<T, V>(a.op[3], n, o, i);
        const GruPack<T, V> cr = gru_load<T, V>(a.op[4], n, o, i), h = gru_load<T, V>(a.op[5], n, o, i);
        GruPack<T, V> gzp, grp, gh;
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const float zf = (float)z.v[k], gr = (float)grh.v[k];
            const float rf = gru_sigmoid((float)rp.v[k] + (float)cr.v[k]);
            const float dz = (1.0f - zf) * zf;
            const float dr = (1.0f - rf) * rf;
            gzp.v[k] = out_cvt<T>((float)gz.v[k] * dz);
            grp.v[k] = out_cvt<T>((gr * (float)h.v[k]) * dr);
            gh.v[k] = out_cvt<T>(gr * rf);
        }
        gru_store<T, V>(a.op[6], n, o, i, gzp);
        gru_store<T, V>(a.op[7], n, o, i, grp);
        gru_store<T, V>(a.op[8], n, o, i, gh);
    }
}

// operands: 0 g_out, 1 z, 2 q_pre, 3 cq, 4 h, 5 g_z, 6 g_qpre, 7 g_h
template <class T, int V>
__global__ __launch_bounds__(256) void gru_blend_bwd_kernel(GruBwdArgs a) {
    const uint32_t step = gridDim.x * 256u;
    for (uint32_t u = blockIdx.x * 256u + threadIdx.x; u < a.units; u += step) {
        const uint32_t row = u / a.J, j = u - row * a.J;
        const uint32_t n = row / a.O, o = row - n * a.O;
        const long long i = (long long)j * V;
        const GruPack<T, V> go = gru_load<T, V>(a.op[0], n, o, i), z = gru_load<T, V>(a.op[1], n, o, i);
        const GruPack<T, V> qp = gru_load<T, V>(a.op[2], n, o, i), cq = gru_load<T, V>(a.op[3], n, o, i);
        const GruPack<T, V> h = gru_load<T, V>(a.op[4], n, o, i);
        GruPack<T, V> gz, gq, gh;
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const float g = (float)go.v[k], zf = (float)z.v[k];
            const float q = tanhf((float)qp.v[k] + (float)cq.v[k]);
            const float dq = 1.0f - q * q;
            gz.v[k] = out_cvt<T>(g * (q - (float)h.v[k]));
            gq.v[k] = out_cvt<T>((g * zf) * dq);
            gh.v[k] = out_cvt<T>(g * (1.0f - zf));
        }
        gru_store<T, V>(a.op[5], n, o, i, gz);
        gru_store<T, V>(a.op[6], n, o, i, gq);
        gru_store<T, V>(a.op[7], n, o, i, gh);
    }
}

template <class T, int V>
static void gru_bwd_launch_v(GruBwdArgs a, bool blend, hipStream_t s) {
    const dim3 g = gru_grid(a, V), t(256);
    if (blend) hipLaunchKernelGGL((gru_blend_bwd_kernel<T, V>), g, t, 0, s, a);
    else hipLaunchKernelGGL((gru_gates_bwd_kernel<T, V>), g, t, 0, s, a);
}

template <class T>
static hipError_t gru_bwd_launch_t(const GruBwdArgs &a, bool blend, hipStream_t s) {
    constexpr int ES = (int)sizeof(T);
    const int bytes = gru_width(a, blend ? 8 : 9, ES);
    if (bytes == 16) gru_bwd_launch_v<T, 16 / ES>(a, blend, s);
    else if (bytes == 8) gru_bwd_launch_v<T, 8 / ES>(a, blend, s);
    else gru_bwd_launch_v<T, 1>(a, blend, s);
    return hipGetLastError();
}

}  // namespace rc

hipError_t rc_launch_gru_bwd(const rc::GruBwdArgs &a, int ek, bool blend, hipStream_t s) {
    if ((long long)a.N * a.O * a.L <= 0) return hipSuccess;
    if (ek == rc::kF32) return rc::gru_bwd_launch_t<float>(a, blend, s);
    if (ek == rc::kF16) return rc::gru_bwd_launch_t<_Float16>(a, blend, s);
    if (ek == rc::kBF16) return rc::gru_bwd_launch_t<__bf16>(a, blend, s);
    return hipErrorInvalidValue;
}
