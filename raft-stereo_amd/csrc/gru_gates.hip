// The elementwise glue of the ConvGRU update (network.py, ConvGRU.forward)
// between its convolutions, as two memory-bound kernels (rc_gru_gates,
// rc_gru_blend; gfx950):
//   gates:  z = sigmoid(z_pre + cz),  r = sigmoid(r_pre + cr);  writes z and r*h
//   blend:  h_out = (1 - z)*h + z*tanh(q_pre + cq)
// The convolutions stay where they are; these replace the adds, sigmoids,
// tanh, multiplies and the two concatenation copies around them.
//
// Every operand is an N x C x HW array addressed by a (batch, channel, pixel)
// stride triple, all of one layout class: planar (pixel stride 1) or
// interleaved (channel stride 1).  Both classes are the same loop here: the
// unit-stride axis is the "inner" axis of length L, the other one the "outer"
// axis of O rows per image, and an operand is (pointer, batch stride, outer
// stride).  A work unit is V consecutive inner elements of one row, moved as
// one access of V * sizeof(T) bytes: 16 where every operand's base and
// strides allow, else 8, else one element (gru_width chooses).
//
// Arithmetic: fp32 on the widened inputs, each operation rounded on its own
// (-ffp-contract=off, like the lookup units), in the order of the PyTorch
// expression; one rounding to T at the store (out_cvt).  The per-element
// functions are shared by every instance, so the vector, scalar, planar and
// interleaved paths give the same bits.
//   sigmoid(a) = 1 / (1 + 2^(-a log2 e)) on the hardware exp2 and reciprocal
//     (1 ulp each): 2^(+inf) = inf gives 0, 2^(-inf) = 0 gives 1, so +-inf and
//     every |a| >= 89 saturate exactly; NaN stays NaN.
//   tanh(a) = tanhf (ocml): +-1 from |a| ~ 9 on and at +-inf, a itself for tiny
//     and subnormal a, NaN for NaN.
// Aliasing: a unit reads all its inputs before it writes, and no other unit
// touches its elements, so z_out may be z_pre and h_out may be h.
#include "gru_gates.h"    // gru_sigmoid, GruPack, gru_load / gru_store, gru_width, gru_grid

namespace rc {

// operands: 0 z_pre, 1 r_pre, 2 cz, 3 cr, 4 h, 5 z_out, 6 rh_out
template <class T, int V>
__global__ __launch_bounds__(256) void gru_gates_kernel(GruArgs a) {
    const uint32_t step = gridDim.x * 256u;
    for (uint32_t u = blockIdx.x * 256u + threadIdx.x; u < a.units; u += step) {
        const uint32_t row = u / a.J, j = u - row * a.J;
        const uint32_t n = row / a.O, o = row - n * a.O;
        const long long i = (long long)j * V;
        const GruPack<T, V> zp = gru_load<T, V>(a.op[0], n, o, i), rp = gru_load<T, V>(a.op[1], n, o, i);
        const GruPack<T, V> cz = gru_load<T, V>(a.op[2], n, o, i), cr = gru_load<T, V>(a.op[3], n, o, i);
        const GruPack<T, V> h = gru_load<T, V>(a.op[4], n, o, i);
        GruPack<T, V> z, rh;
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const float zf = gru_sigmoid((float)zp.v[k] + (float)cz.v[k]);
            const float rf = gru_sigmoid((float)rp.v[k] + (float)cr.v[k]);
            z.v[k] = out_cvt<T>(zf);
            rh.v[k] = out_cvt<T>(rf * (float)h.v[k]);
        }
        gru_store<T, V>(a.op[5], n, o, i, z);
        gru_store<T, V>(a.op[6], n, o, i, rh);
    }
}

// operands: 0 z, 1 q_pre, 2 cq, 3 h, 4 h_out
template <class T, int V>
__global__ __launch_bounds__(256) void gru_blend_kernel(GruArgs a) {
    const uint32_t step = gridDim.x * 256u;
    for (uint32_t u = blockIdx.x * 256u + threadIdx.x; u < a.units; u += step) {
        const uint32_t row = u / a.J, j = u - row * a.J;
        const uint32_t n = row / a.O, o = row - n * a.O;
        const long long i = (long long)j * V;
        const GruPack<T, V> z = gru_load<T, V>(a.op[0], n, o, i), qp = gru_load<T, V>(a.op[1], n, o, i);
        const GruPack<T, V> cq = gru_load<T, V>(a.op[2], n, o, i), h = gru_load<T, V>(a.op[3], n, o, i);
        GruPack<T, V> out;
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const float zf = (float)z.v[k];
            const float q = tanhf((float)qp.v[k] + (float)cq.v[k]);
            const float keep = (1.0f - zf) * (float)h.v[k];
            const float take = zf * q;
            out.v[k] = out_cvt<T>(keep + take);
        }
        gru_store<T, V>(a.op[4], n, o, i, out);
    }
}

template <class T, int V>
static void gru_launch_v(GruArgs a, bool blend, hipStream_t s) {
    const dim3 g = gru_grid(a, V), t(256);
    if (blend) hipLaunchKernelGGL((gru_blend_kernel<T, V>), g, t, 0, s, a);
    else hipLaunchKernelGGL((gru_gates_kernel<T, V>), g, t, 0, s, a);
}

template <class T>
static hipError_t gru_launch_t(const GruArgs &a, bool blend, hipStream_t s) {
    constexpr int ES = (int)sizeof(T);
    const int bytes = gru_width(a, blend ? 5 : 7, ES);
    if (bytes == 16) gru_launch_v<T, 16 / ES>(a, blend, s);
    else if (bytes == 8) gru_launch_v<T, 8 / ES>(a, blend, s);
    else gru_launch_v<T, 1>(a, blend, s);
    return hipGetLastError();
}

}  // namespace rc

hipError_t rc_launch_gru(const rc::GruArgs &a, int ek, bool blend, hipStream_t s) {
    if ((long long)a.N * a.O * a.L <= 0) return hipSuccess;
    if (ek == rc::kF32) return rc::gru_launch_t<float>(a, blend, s);
    if (ek == rc::kF16) return rc::gru_launch_t<_Float16>(a, blend, s);
    if (ek == rc::kBF16) return rc::gru_launch_t<__bf16>(a, blend, s);
    return hipErrorInvalidValue;
}
