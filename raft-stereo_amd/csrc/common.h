// Internal helpers shared by the gfx950 kernels and the C-ABI layer.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#ifdef RAFTCORR_DEV
#include <stdlib.h>
#endif

namespace rc {

// Dev-only A/B knobs (environment variables read per launch).  They exist
// only in libraftcorr_dev.so (built with -DRAFTCORR_DEV, tools/ablate.py);
// the product library has no knobs, no getenv and no ablation kernels.
#ifdef RAFTCORR_DEV
inline int dev_knob(const char *name) {
    const char *e = getenv(name);
    return e ? atoi(e) : 0;
}
#endif

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

constexpr int kMaxLevels = 8;

// Correctly rounded a / b for the sampler's normalisation xn = 2x/(W-1) - 1
// (model.py:271), with b = W - 1 a positive integer.  rb = RN(1/b) is computed
// once per level; per tap Markstein's correction q0 = RN(a*rb) (within 1 ulp
// of a/b), r = a - q0*b (exact with fma), q = RN(q0 + r*rb) = RN(a/b)
// (Markstein, IBM J. R&D 34(1), 1990; Muller et al., Handbook of
// Floating-Point Arithmetic, ch. 4) costs 3 VALU ops instead of the ~10-op
// IEEE division sequence with its quarter-rate v_rcp.  tests/test_div_rn.py
// checks it bit for bit against IEEE division on gfx950 for EVERY b in
// [1, 8192] and every fp32 a with 2^-30 <= |a| < 2^15, and for sampled wider
// b.  Outside that a-range a difference could not reach the sampler's output:
// |a| < 2^-30 gives |q| < 2^-25, so xn = q - 1 rounds to -1 either way, and
// |a| > 2(W + R + 2) puts every tap outside the row (zeros).  A NaN/inf
// numerator gives NaN where division gives +-inf; the sampler turns both into
// the same NaN output (W = 1, b = 0, likewise: (xn + 1) * 0 is NaN both ways).
struct DivRN {
    float b, rb;
};
__device__ __forceinline__ DivRN div_prep(float b) { return DivRN{b, 1.0f / b}; }
__device__ __forceinline__ float div_rn(float a, const DivRN &d) {
    const float q0 = a * d.rb;
    const float r = __builtin_fmaf(-q0, d.b, a);
    return __builtin_fmaf(r, d.rb, q0);
}

// XCD-aware bijective block remap: hardware workgroup v runs on XCD v % 8, so
// give XCD x the contiguous logical range [x*q + min(x, n%8), ...) of the n
// blocks: neighbouring logical blocks then share an XCD (and its L2).
__device__ __forceinline__ int xcd_remap(int v, int n) {
    const int xcd = v & 7, q = n >> 3, rr = n & 7;
    return (xcd < rr ? xcd * (q + 1) : rr * (q + 1) + (xcd - rr) * q) + (v >> 3);
}

// Raw buffer resource over [base, base + bytes): loads past the end (or at a
// "negative" offset, which wraps to a huge unsigned one) return 0 and never
// fault.  Build it from wave-uniform values only (cdna_hip_programming.md T20).
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void *base, uint32_t bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(base), (short)0, (int)bytes,
                                             0x00020000);
}

__device__ __forceinline__ f32x4 ld4(__amdgpu_buffer_rsrc_t r, uint32_t byte_off) {
    return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, (int)byte_off, 0, 0));
}

__device__ __forceinline__ float ld1(__amdgpu_buffer_rsrc_t r, uint32_t byte_off) {
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, (int)byte_off, 0, 0));
}

__device__ __forceinline__ uint32_t clamp_bytes(long long n) {
    return n <= 0 ? 0u : (n > 0xFFFFFF00LL ? 0xFFFFFF00u : (uint32_t)n);
}

// bf16 helpers (round-to-nearest-even; NaN stays NaN via the hardware cvt).
__device__ __forceinline__ float bf16_to_f32(uint16_t v) {
    return __builtin_bit_cast(float, (uint32_t)v << 16);
}
__device__ __forceinline__ uint16_t f32_to_bf16(float f) {
    __bf16 b = (__bf16)f;
    return __builtin_bit_cast(uint16_t, b);
}
// fp32 value rounded to bf16 precision (RNE), kept in fp32.
__device__ __forceinline__ float round_bf16(float f) { return bf16_to_f32(f32_to_bf16(f)); }

// Element kind of a pyramid (or of 16-bit feature maps): the C-ABI's RC_F32 /
// RC_BF16 / RC_F16 codes.  A `bool bf16` of older code converts to kF32 / kBF16.
enum : int { kF32 = 0, kBF16 = 1, kF16 = 2 };

// fp16 helpers: the hardware convert (v_cvt_f16_f32) rounds to nearest even,
// keeps +-inf, overflows to +-inf above 65504 and keeps subnormals (the
// kernels' fp16 denormal mode is IEEE) -- what Tensor.half() does.  The
// opaque copy keeps the fp32 value a value of its own: the compiler may not
// fold the multiply that made it and this convert into one v_fma_mixlo_f16
// (one rounding instead of two; see out_cvt in lookup_pair.h).
__device__ __forceinline__ float f16_to_f32(uint16_t v) { return (float)__builtin_bit_cast(_Float16, v); }
__device__ __forceinline__ uint16_t f32_to_f16(float f) {
    asm("" : "+v"(f));
    return __builtin_bit_cast(uint16_t, (_Float16)f);
}
__device__ __forceinline__ float round_f16(float f) { return f16_to_f32(f32_to_f16(f)); }

// The same three for an element kind EK (kBF16 or kF16), compile-time or not.
__device__ __forceinline__ float h16_to_f32(uint16_t v, int ek) { return ek == kF16 ? f16_to_f32(v) : bf16_to_f32(v); }
__device__ __forceinline__ uint16_t f32_to_h16(float f, int ek) { return ek == kF16 ? f32_to_f16(f) : f32_to_bf16(f); }
__device__ __forceinline__ float round_h16(float f, int ek) { return ek == kF16 ? round_f16(f) : round_bf16(f); }
// the two halves of a packed pair, widened
__device__ __forceinline__ float h16_lo(uint32_t u, int ek) {
    return ek == kF16 ? f16_to_f32((uint16_t)u) : __builtin_bit_cast(float, u << 16);
}
__device__ __forceinline__ float h16_hi(uint32_t u, int ek) {
    return ek == kF16 ? f16_to_f32((uint16_t)(u >> 16)) : __builtin_bit_cast(float, u & 0xFFFF0000u);
}

// v / sqrt(D) as the reference's division (model.py:326): a multiply by the
// exact 1/sqrt(D) when D is a power of four (a.pow2), the correctly rounded
// division otherwise.  One wave-uniform branch around the whole group: the
// empty volatile asm keeps the division path a real branch, so the
// power-of-two path never evaluates it (a select per element would).
template <int N, class Args>
__device__ __forceinline__ void apply_scale(float (&v)[N], const Args &a) {
    if (a.pow2) {
#pragma unroll
        for (int k = 0; k < N; ++k) v[k] *= a.scale;
    } else {
        asm volatile("");
#pragma unroll
        for (int k = 0; k < N; ++k) v[k] = v[k] / a.sq;
    }
}

// Kernel parameter blocks (passed by value).
struct BuildArgs {
    const void *f1, *f2;      // [B][D][H][W1], [B][D][H][W2]
    void *lvl[kMaxLevels];    // pyramid outputs
    long long ld[kMaxLevels]; // their row strides (elements, >= W2 >> l)
    int B, D, H, W1, W2;
    int nfused;               // levels written by the epilogue (1..7)
    int tiles_m, tiles_n;     // 128x128 workgroup tiles per (b,h) row
    float scale;              // exact reciprocal of sqrt(D) when pow2 != 0
    float sq;                 // sqrtf(D)
    int pow2;                 // sqrt(D) is a power of two -> multiply is exact
    int pyr_bf16;             // pyramid element kind: kF32, kBF16 or kF16 (non-zero: a 16-bit pyramid)
    int stagger;              // reserved (no reader): keeps the kernarg offsets of the fields below
    // line-phase shadow copies (ABI v5, RC_SHADOW): a stored level l is also
    // written at (char*)lvl[l] + shadow[l] bytes (0 = no copy)
    long long shadow[kMaxLevels];
    // RC_LAYOUT_DISPARITY (ABI v9): levels 0 and 2 disparity-major, shk[l]
    // rows (diagonals) of ld[l] elements per row block; 0 = row layout
    long long shk[kMaxLevels];
    // RC_LAYOUT_RECORDS (ABI v10): levels 0 and 2 as rec_nr 128-B records
    // per pixel row at rec (the bf16 ring build's deferred epilogue)
    void *rec;
    int rec_nr;
};

// RC_LAYOUT_RECORDS geometry (include/raftcorr.h): record r of a pixel row
// holds level-2 elements 4r - 14 .. 4r + 11 in slots 0..25 and level-0
// elements 16r - 26 .. 16r + 11 in slots 26..63 (bf16), so a pixel whose
// level-1 centre floor(x/2) lies in [8r - 8, 8r) finds the spans of all four
// levels (radius <= 4) in that one line.
constexpr int kRecSlots = 64, kRecL2Slots = 26;
constexpr int kRecM0 = -8;                       // level-1 centre of record 0's first pixel
__host__ __device__ constexpr int rec_e0(int r) { return 16 * r + 2 * kRecM0 - 10; }   // first level-0 element
__host__ __device__ constexpr int rec_e2(int r) { return 4 * r + kRecM0 / 2 - 10; }    // first level-2 element

struct LookupArgs {
    const void *lvl[kMaxLevels];
    int W[kMaxLevels];
    long long ld[kMaxLevels]; // row strides (elements, >= W)
    const float *coords;
    long long cbs;            // coords batch stride (elements)
    float *out;
    long long P;              // B*H*W1
    int HW;                   // H*W1
    int levels;
    // rc_corr_lookup_step only (step != 0): coords is the whole (B,2,H,W1)
    // coords1; x = coords1.x + delta.x (delta may be null), and the advanced
    // coords and flow = coords - coords_grid are written before the lookup
    int step;
    int W1;
    const float *delta;
    float *coords_out;
    float *flow_out;
    // line-phase shadow copy of level i at (char*)lvl[i] + shadow[i] bytes
    // (0 = none); read by the pair kernel (RC_SHADOW, ABI v5)
    long long shadow[kMaxLevels];
    int out_cl;               // channels-last output out[p*C + ch] (pair kernel; ABI v5)
    // RC_LAYOUT_DISPARITY (ABI v9): levels 0 and 2 disparity-major, shk[l]
    // rows (diagonals) of ld[l] elements per row block; 0 = row layout
    long long shk[kMaxLevels];
    // RC_LAYOUT_RECORDS (ABI v10): lvl[0] = the records, rec_nr per pixel row
    int rec_nr;
    // RC_OUT_F16 / RC_OUT_BF16 (ABI v13): out holds 1 = fp16, 2 = bf16 elements
    // (pair and records kernels only, lookup_half.hip); 0 = fp32
    int out_dt;
};

// Backward of the lookup: level gradients (fp32, row stride ld[i] % 4 == 0).
struct LookupBwdArgs {
    float *g[kMaxLevels];
    int W[kMaxLevels];
    long long ld[kMaxLevels];
    const float *coords;
    long long cbs;
    const float *grad_out;    // [B][levels*(2r+1)][H][W1]
    long long P;
    int HW;
    int levels;
    long long shadow[kMaxLevels];   // bytes from g[l] to its RC_SHADOW copy (pair layout), 0 = none
};

// Deferred lookup backward (backward_calls.hip): the gradients of up to
// kMaxBwdCalls lookup calls summed into pair-layout buffers in one pass.
constexpr int kMaxBwdCalls = 32;
struct LookupBwdCallsArgs {
    float *g[2];              // level 0 and level 2 gradient rows (pair layout)
    long long ld[2];          // their row strides (floats, % 4 == 0)
    int W[4];                 // level widths W0 >> l
    int wout[2];              // columns written back per row (round4(W), <= ld)
    int rowbase[2];           // LDS float offset of row 0, element 0, of pair k
    int S[2];                 // LDS row stride (floats) of pair k
    int lds_floats;           // LDS floats zeroed per workgroup (% 4 == 0)
    int pix;                  // pixels per workgroup
    int ncalls;               // 1..kMaxBwdCalls
    int accumulate;           // 0: overwrite the rows; 1: add to them
    int budget;               // compact kernel: LDS floats per block (one wave)
    long long P;
    int HW;
    const float *coords[kMaxBwdCalls];
    long long cbs[kMaxBwdCalls];
    const float *grad_out[kMaxBwdCalls];   // [B][levels*(2r+1)][H][W1]
};

// Backward of the build: level gradients -> feature-map gradients (fp32).
struct BuildBwdArgs {
    const float *f1, *f2;     // [B][D][H][W1], [B][D][H][W2]
    const float *g[kMaxLevels];
    long long ld[kMaxLevels]; // level-gradient row strides (ld[0] % 4 == 0)
    int Wl[kMaxLevels];       // level widths W2 >> l
    int nlev;
    float *df1, *df2;         // outputs, layouts of f1 / f2
    int B, D, H, W1, W2;
    int tm, tn1, tn2;         // 128-row d tiles; 128-col tiles over W1 (dF1) / W2 (dF2)
    float scale, sq;
    int pow2;
    long long shadow[kMaxLevels];   // floats from g[l] to its RC_SHADOW copy (kPairFold), 0 = none
    int exact;                      // 1: exact fp32 MFMA kernel (RC_BUILD_EXACT_F32); 0: split-bf16
    int dev_only;                   // dev library timing probe: 1 = dF1 tiles only, 2 = dF2 only
};

// rc_gru_gates / rc_gru_blend (gru_gates.hip).  An operand is N images of O
// rows of L unit-stride elements: the rows are channels and the elements
// pixels for the planar layout class, pixels and channels for the interleaved
// one.  Strides in elements.
struct GruOperand {
    void *p;
    long long sn, so;         // batch stride, row stride
};
struct GruArgs {
    GruOperand op[7];         // gates: z_pre r_pre cz cr h z_out rh_out; blend: z q_pre cq h h_out
    int N;
    uint32_t O;
    long long L;
    uint32_t J, units;        // set by the launcher: work units per row, and in all (< 2^32)
};
// rc_gru_gates_backward / rc_gru_blend_backward (gru_gates_bwd.hip): the same
// with room for their 9 / 8 operands (GruArgs keeps its size, and with it the
// forward kernels their code).
struct GruBwdArgs {
    GruOperand op[9];         // gates: g_z g_rh z r_pre cr h g_zpre g_rpre g_h
                              // blend: g_out z q_pre cq h g_z g_qpre g_h
    int N;
    uint32_t O;
    long long L;
    uint32_t J, units;
};

// rc_gru_assemble (gru_inputs.hip): the [h, x] buffer filled from up to
// kGruMaxParts sources, each copied, 3x3/2 average-pooled or bilinearly resized
// into its channel range.  Strides in elements, (batch, channel, row, column).
constexpr int kGruMaxParts = 4;
enum : int { kPartCopy = 0, kPartPool2x = 1, kPartBilinear = 2 };
struct GruPart {
    const void *p;
    long long sn, sc, sh, sw;
    int c0, C;                // its channels of dst: [c0, c0 + C)
    int mode, ek;             // kPart*, element kind
    int SH, SW;               // source height and width
    float scale_h, scale_w;   // bilinear: (S - 1) / (D - 1) per axis, 0 for D == 1
};
struct GruAsmArgs {
    void *dst;
    long long dn, dc, dh, dw;
    int N, C, H, W;           // C: the channels of all parts
    int nparts;
    uint32_t J, units;        // set by the launcher: work units per pixel (interleaved) or row (planar), and in all
    int cend[kGruMaxParts];   // c0 + C of part i; C of an absent one
    GruPart part[kGruMaxParts];
};

// rc_gru_assemble_backward (gru_inputs_bwd.hip): the adjoint.  G = g (+ g2 from
// channel g2_c0 on) is the gradient of the assembled buffer, part i's output
// the gradient of its source.  A part without an output (p == nullptr) has no
// units; its channels still count in c0.
struct GruBwdPart {
    void *p;
    long long sn, sc, sh, sw;
    int c0, C;                // its channels of G: [c0, c0 + C)
    int mode, ek;             // kPart*, the output's element kind
    int SH, SW;               // the output's (the source's) height and width
    float scale_h, scale_w;   // as GruPart's
    uint32_t J;               // set by the launcher: units per pixel (interleaved) or row (planar)
    unsigned long long u0;    // set by the launcher: the part's first unit
};
struct GruAsmBwdArgs {
    const void *g, *g2;       // g2 may be null
    long long gn, gc, gh, gw;
    int g2_c0;
    int N, C, H, W;           // of G
    int nparts;
    unsigned long long units;                  // set by the launcher: all parts'
    unsigned long long uend[kGruMaxParts];     // set by the launcher: u0 + units of part i
    GruBwdPart part[kGruMaxParts];
};

// rc_upsample_head (upsample_head.hip).  Strides in elements; the mask's other
// two strides are its layout class's (planar: H W per channel, 1 per pixel;
// interleaved: 1 and 9 f^2).
struct HeadArgs {
    const float *flow;
    long long fsn, fsc;       // flow batch and channel strides (pixel stride 1)
    const void *mask;
    long long msn;            // mask batch stride
    float scale;
    float *out;               // [N][C][f H][f W]
    int N, C, H, W;
    long long groups;         // set by the launcher: lanes per sub-row
};

// CUs of the device current at the first call, taken once: every GPU of a
// node this project runs on is the same.  256 when the query fails.
inline int device_cus() {
    static const int ncu = [] {
        int d = 0, n = 0;
        if (hipGetDevice(&d) != hipSuccess ||
            hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, d) != hipSuccess || n <= 0)
            n = 256;
        return n;
    }();
    return ncu;
}

}  // namespace rc

// Host-side launchers (defined in the .hip files, called by capi.cpp).
hipError_t rc_launch_build_f32(const rc::BuildArgs &a, hipStream_t s);
hipError_t rc_launch_build_split(rc::BuildArgs &a, hipStream_t s);     // may lower a.nfused
// in_16: the fmaps hold 16-bit elements of the pyramid's kind (a.pyr_bf16), else fp32
hipError_t rc_launch_build_bf16mma(rc::BuildArgs &a, int in_16, hipStream_t s);   // may lower a.nfused
// the same for an fp16 pyramid (a.pyr_bf16 == kF16; volume_half.hip)
hipError_t rc_launch_build_f16mma(rc::BuildArgs &a, int in_16, hipStream_t s);
// ek: element kind (kF32 / kBF16 / kF16)
hipError_t rc_launch_pool(const void *in, long long ld_in, void *out, long long ld_out, long rows,
                          int W_in, int ek, hipStream_t s);
hipError_t rc_launch_lookup(const rc::LookupArgs &a, int radius, int pyr_bf16, hipStream_t s);
hipError_t rc_launch_lookup_conv(const rc::LookupArgs &a, int radius, int pyr_bf16, const float *w,
                                 const float *b, int cout, int relu, float *out, hipStream_t s);
// grad_corr / grad_weight / grad_bias may be null (not computed); workspace is
// used only when grad_weight or grad_bias is given
hipError_t rc_launch_lookup_conv_bwd(const rc::LookupArgs &a, int radius, int pyr_bf16, const float *w,
                                     const float *b, int cout, int relu, const float *grad_out,
                                     float *grad_corr, float *grad_weight, float *grad_bias,
                                     float *workspace, hipStream_t s);
// the fused lookup + convc1 on the pair layout (lookup_pair_conv.hip): a.out holds [B][cout][H][W1]
// elements of a.out_dt; the backward takes rc_launch_lookup_conv_bwd's arguments
hipError_t rc_launch_lookup_pair_conv(const rc::LookupArgs &a, int radius, int pyr_bf16, const float *w,
                                      const float *b, int cout, int relu, hipStream_t s);
hipError_t rc_launch_lookup_pair_conv_bwd(const rc::LookupArgs &a, int radius, int pyr_bf16, const float *w,
                                          const float *b, int cout, int relu, const float *grad_out,
                                          float *grad_corr, float *grad_weight, float *grad_bias,
                                          float *workspace, hipStream_t s);
hipError_t rc_launch_lookup_chain(const rc::LookupArgs &a, int radius, hipStream_t s);
hipError_t rc_launch_lookup_pair(const rc::LookupArgs &a, int radius, int pyr_bf16, hipStream_t s);
// the pair / records kernels with a.out_dt != 0 (called by rc_launch_lookup_pair; lookup_half.hip)
hipError_t rc_launch_lookup_pair_half(const rc::LookupArgs &a, int radius, int pyr_bf16, hipStream_t s);
// an fp16 pyramid (RC_F16; lookup_f16pyr.hip): the per-level lookup and the pair lookup, every a.out_dt
hipError_t rc_launch_lookup_f16pyr(const rc::LookupArgs &a, int radius, hipStream_t s);
hipError_t rc_launch_lookup_pair_f16pyr(const rc::LookupArgs &a, int radius, hipStream_t s);
hipError_t rc_launch_lookup_bwd(const rc::LookupBwdArgs &a, int radius, hipStream_t s);
// fills a.pix / rowbase / S / lds_floats from W, radius, levels
hipError_t rc_launch_lookup_bwd_calls(rc::LookupBwdCallsArgs &a, int radius, int levels, hipStream_t s);
bool rc_lookup_bwd_calls_fits(const rc::LookupBwdCallsArgs &a, int radius, int levels, const long *cbs,
                              int n_calls);
hipError_t rc_launch_volume_bwd(const rc::BuildBwdArgs &a, hipStream_t s);
// the ConvGRU gate / blend kernel on operands of element kind ek (gru_gates.hip)
hipError_t rc_launch_gru(const rc::GruArgs &a, int ek, bool blend, hipStream_t s);
// their backward kernels (gru_gates_bwd.hip)
hipError_t rc_launch_gru_bwd(const rc::GruBwdArgs &a, int ek, bool blend, hipStream_t s);
// the ConvGRU input assembly into a dst of element kind ek, planar or
// interleaved (gru_inputs.hip); sets a.J and a.units
hipError_t rc_launch_gru_assemble(rc::GruAsmArgs &a, int ek, bool interleaved, hipStream_t s);
// its adjoint from a G of element kind ek (gru_inputs_bwd.hip); sets the unit counts of a
hipError_t rc_launch_gru_assemble_bwd(rc::GruAsmBwdArgs &a, int ek, bool interleaved, hipStream_t s);
hipError_t rc_launch_convex_upsample(const float *flow, const float *mask, int N, int C, int H,
                                     int W, int factor, float *out, hipStream_t s);
// grad_flow / grad_mask may be null (not computed); workspace is read only with grad_flow
hipError_t rc_launch_convex_upsample_bwd(const float *flow, const float *mask, const float *grad_out,
                                         int N, int C, int H, int W, int factor, float *grad_flow,
                                         float *grad_mask, float *workspace, hipStream_t s);
// rc_upsample_head's kernel on a mask of element kind ek, planar or interleaved
// (upsample_head.hip); picks the access width and sets a.groups
hipError_t rc_launch_upsample_head(rc::HeadArgs &a, int ek, int factor, bool interleaved, hipStream_t s);
