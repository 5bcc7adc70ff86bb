/*
 * raftcorr.h -- C-ABI of the MI355X (gfx950) correlation path for RAFT-Stereo.
 *
 * Drop-in boundary for the reference's CorrBlock1D (/root/reference/model.py):
 *   rc_corr_build   replaces CorrBlock1D.__init__ + CorrBlock1D.corr
 *                   (model.py:284-295 and :318-326): all-pairs per-row volume
 *                   / sqrt(D) plus the avg-pooled pyramid, in one launch.
 *   rc_corr_pool    replaces one F.avg_pool2d([1,2]) pyramid step (model.py:294);
 *                   used for levels beyond the fused epilogue (and for A/B runs).
 *   rc_corr_lookup  replaces CorrBlock1D.__call__ + bilinear_sampler
 *                   (model.py:297-316 and :267-281).
 *   rc_corr_lookup_conv  the lookup fused with BasicMotionEncoder.convc1 +
 *                   ReLU (model.py:199, :206), SURVEY.md §8f rank 1.
 *   rc_corr_lookup_conv_backward  its gradient with respect to the
 *                   correlation, the conv weight and the bias, for training
 *                   with the fused layer (the lookup is recomputed).
 *   rc_corr_lookup_chain_conv, rc_corr_lookup_chain_conv_backward  the same
 *                   fused layer and its gradient on the PAIR layout (levels
 *                   0 and 2 stored, 1 and 3 derived in registers), with an
 *                   fp32, fp16 or bf16 output: what CorrBlock1D stores by
 *                   default, so nothing is pooled for the fused path.
 *   rc_corr_lookup_chain rc_corr_lookup for a pool-chain fp32 pyramid,
 *                   reading levels 0-1 only (the default of CorrBlock1D).
 *   rc_corr_lookup_step  coords update + flow + lookup of one loop
 *                   iteration in one launch.
 *   rc_convex_upsample  the convex upsampler for the mask the update block
 *                   produces.
 *   rc_convex_upsample_backward  its gradient with respect to flow and mask,
 *                   for a training loss on the full-resolution prediction.
 *   rc_upsample_head  the same upsampler for an inference forward's last
 *                   step: an fp32, fp16 or bf16 mask, NCHW or channels-last,
 *                   scaled inside the kernel.
 *   rc_corr_lookup_backward, rc_corr_build_backward  the gradient of the
 *                   path to the feature maps (autograd of model.py:267-326),
 *                   SURVEY.md §8f rank 2.
 *   rc_gru_gates, rc_gru_blend and their backwards  the elementwise glue of
 *                   ConvGRU.forward (model.py:164-179) between its convolutions.
 *   rc_gru_assemble the work in front of each ConvGRU call: pool2x and interp
 *                   (model.py:182-186) and the concatenation of [h, x]
 *                   (model.py:172-173), one launch, nothing in between stored.
 *   rc_gru_assemble_backward  its adjoint: the gradients of every part's source
 *                   from the gradient(s) of the buffer, one launch, no atomics.
 *
 * The reference has no FFI; its "operator API" is the duck-typed class bound
 * at model.py:366-367 and called at :376.  raft-stereo_amd/corr.py mirrors that
 * class on top of these entry points (ctypes).
 *
 * Conventions: plain pointers and sizes, device pointers from any allocator
 * (PyTorch's caching allocator in practice), stream = hipStream_t passed as
 * void* (NULL = default stream).  Nothing is allocated, nothing synchronises,
 * nothing throws across the ABI.  Return 0 on success, else an RC_E* code;
 * rc_last_error() then describes the failure (thread-local).
 */
#ifndef RAFTCORR_H
#define RAFTCORR_H

#ifdef __cplusplus
extern "C" {
#endif

/* Version 13 also covers rc_corr_lookup_chain_conv and
 * rc_corr_lookup_chain_conv_backward: they were added without changing any
 * existing entry point, flag or layout (purely additive), so the number did
 * not move.  A caller that needs them checks for the symbols.
 * The element type RC_F16 was added the same way: a new value of an existing
 * argument that a version-13 caller never passes (a library from before it
 * answers RC_EINVAL "unknown dtype"), no entry point, flag or layout changed,
 * so the number did not move for it either.  rc_gru_gates / rc_gru_blend and
 * their backward entry points are additive in the same way, and so is
 * rc_gru_assemble with rc_gru_assemble_backward, and rc_upsample_head. */
#define RC_ABI_VERSION 13

/* element types */
#define RC_F32  0
#define RC_BF16 1
/* IEEE fp16.  An fp16 pyramid is the bf16 pyramid's twin for an fp16-autocast
 * network: the same bytes, 11 significant bits instead of 8, built on
 * v_mfma_f32_16x16x32_f16 (the bf16 instruction's rate).  Level 0 is the fp32
 * accumulator / sqrtf(D) rounded once to nearest even (fp16 subnormals kept,
 * magnitudes above 65504 become +-inf: fp16 has 5 exponent bits where bf16 has
 * 8); every higher level is fp16((x + y) * 0.5f) of the level below AS STORED
 * (so +inf and -inf pool to NaN).  Accepted by
 *   rc_corr_build         (fmap RC_F16, pyr RC_F16) and (fmap RC_F32, pyr
 *                         RC_F16: fmaps rounded to fp16 on load), RC_SHADOW_LEVEL
 *                         bits as for bf16;
 *   rc_corr_pool;
 *   rc_corr_lookup        (every level stored);
 *   rc_corr_lookup_chain  on the pair layout only, as for bf16 (2 levels, or 4
 *                         with levels 0 and 2 stored), with RC_SHADOW,
 *                         RC_OUT_CHANNELS_LAST and RC_OUT_F16 / RC_OUT_BF16.
 * RC_EUNSUPPORTED, before any launch, for: an fp32 pyramid from fp16 fmaps,
 * any fp16 / bf16 mix, RC_LAYOUT_RECORDS, RC_LAYOUT_DISPARITY and
 * RC_BUILD_EXACT_F32 in rc_corr_build; and as the pyramid type of every other
 * entry point (rc_corr_lookup_step, rc_corr_lookup_conv,
 * rc_corr_lookup_chain_conv and their backwards).  rc_corr_build_backward is
 * unchanged: it takes fp32 fmaps (widen fp16 ones). */
#define RC_F16  2

/* Flags OR-ed into a pyr_dtype argument (ABI v5): RC_SHADOW_LEVEL(l) says
 * stored pyramid level l has a line-phase SHADOW copy (RC_SHADOW: every
 * stored level) -- the same rows, at byte offset
 * RC_SHADOW_OFFSET(rows, ld, esize) from the level's base (rows = B*H*W1,
 * ld = its row stride in elements, esize = 4 for RC_F32, 2 for RC_BF16 / RC_F16), so
 * the allocation holds rows*ld*esize bytes, a gap, then the copy, shifted by
 * half a 128-byte line against the primary when the base is 128-B aligned.
 * rc_corr_build writes both copies; the pair kernel of rc_corr_lookup_chain /
 * rc_corr_lookup_step reads each pixel's span from the copy in which it
 * touches fewer 128-B lines (bit-identical results, fewer HBM lines per
 * pixel).  The other entry points accept the flag and read the primary copy.
 * A level and its copy must fit in 4 GiB (RC_EUNSUPPORTED otherwise).  The
 * copies cost build-time writes; which levels pay for themselves depends on
 * the level's size and how often it is read. */
#define RC_SHADOW_LEVEL(l) (0x100 << (l))
#define RC_SHADOW 0xFF00
#define RC_SHADOW_OFFSET(rows, ld, esize) \
    ((((long long)(rows) * (long long)(ld) * (long long)(esize) + 127) / 128) * 128 + 64)

/* Flag OR-ed into the pyr_dtype of rc_corr_lookup_chain / rc_corr_lookup_step
 * (ABI v5): write the lookup output channels-last, out[((b*H + h)*W1 + w)*C + c]
 * with C = levels*(2r+1) -- the (B, C, H, W1) tensor in NHWC memory order
 * (torch.channels_last), the same values.  Pair kernel only (2 levels, or 4
 * with level 2 given); RC_EUNSUPPORTED otherwise. */
#define RC_OUT_CHANNELS_LAST 0x10000

/* Flags OR-ed into the pyr_dtype of rc_corr_lookup_chain / rc_corr_lookup_step
 * (ABI v13): `out` holds IEEE fp16 (RC_OUT_F16) or bfloat16 (RC_OUT_BF16)
 * elements instead of fp32, in the same shape and channel order (with or
 * without RC_OUT_CHANNELS_LAST) -- the dtype a mixed-precision consumer would
 * cast the fp32 output to.  Each element is the fp32 result of the call
 * without the flag, rounded to nearest even by the hardware convert: +-inf
 * stays +-inf, fp16 overflow gives +-inf, fp16 subnormal results are kept
 * (not flushed), NaN gives a NaN of that type (payload and sign unspecified).
 * coords1_out and flow_out of rc_corr_lookup_step stay fp32.  Served where
 * the pair kernel or the records kernel runs: 2 levels, or 4 with level 2
 * given, or RC_LAYOUT_RECORDS (chain != 0 in the step), any shadow copies.
 * RC_EUNSUPPORTED before any launch otherwise (the level-1 chain,
 * RC_LAYOUT_DISPARITY, chain == 0, every other entry point); both flags
 * together are RC_EINVAL. */
#define RC_OUT_F16  0x40000
#define RC_OUT_BF16 0x200000

/* Flag OR-ed into the pyr_dtype of rc_corr_build (ABI v6): run the exact fp32
 * MFMA kernel (v_mfma_f32_16x16x4_f32) for fp32 fmaps and an fp32 pyramid.
 * Without it such a build runs the split-bf16 kernel: every fp32 operand is
 * the exact sum of three bf16 pieces and each product the sum of the six
 * leading piece products on v_mfma_f32_16x16x32_bf16 with fp32 accumulation
 * -- fp32 accuracy (measured at or below the fp32 MFMA chain's error against
 * an fp64 volume) at a third of the MFMA time.  Non-finite fmap values are
 * the exception: an inf operand gives NaN in its row's volume where the fp32
 * GEMM gives +-inf; pass this flag for such inputs.  Ignored by bf16 builds. */
#define RC_BUILD_EXACT_F32 0x20000

/* Flag OR-ed into the pyr_dtype of rc_corr_build and rc_corr_lookup_chain
 * (ABI v9): the pair layout's stored levels -- level 0, and level 2 of a
 * 4-level pyramid (pyr[1] == NULL) -- are DISPARITY-MAJOR.  Level l of row
 * block r = b*H + h is an array S of RC_SHEAR_ROWS(W2, W1, l) rows of
 * pyr_ld[l] fp32 elements (pyr_ld[l] >= W1, a multiple of 4), at
 * pyr[l] + r * RC_SHEAR_ROWS(W2, W1, l) * pyr_ld[l], with
 *     S[k][w1] = C_l[(r, w1)][j],   k = (w1 >> l) - j + (W2 >> l) - 1,
 * so the pixels of an image row that look at the same disparity read one
 * contiguous run of a row of S.  Entries with j outside [0, W2 >> l) are
 * neither written nor read.  The values are the row layout's bit for bit and
 * so are the lookups (rc_corr_lookup_chain with the flag: the pair kernel's
 * arithmetic); it pays where neighbouring pixels' coords agree (the
 * network's fields), and loses on independent random coords (DESIGN.md
 * §3.2h).  Requires fp32 fmaps and pyramid on the split-bf16 build (W1, W2
 * multiples of 4, no RC_BUILD_EXACT_F32, no shadow copies), nbuf 1 (2 levels)
 * or 3 with pyr[1] == NULL (4 levels), radius 1..4, NCHW output, each level
 * under 4 GiB; RC_EUNSUPPORTED otherwise.  The other entry points refuse it. */
#define RC_LAYOUT_DISPARITY 0x80000
#define RC_SHEAR_ROWS(W2, W1, l) (((W2) >> (l)) + (((W1) - 1) >> (l)))

/* Flag OR-ed into the pyr_dtype of rc_corr_build, rc_corr_lookup_chain and
 * rc_corr_lookup_step (ABI v10): the 4-level bf16 pair layout's stored levels
 * 0 and 2 as RECORDS -- one 128-byte line per pixel per lookup instead of two
 * (DESIGN.md §3.2i).  pyr[0] is the record buffer: B*H*W1 pixel rows of
 * RC_REC_COUNT(W2) records of RC_REC_SLOTS bf16 (RC_REC_BYTES each, pixel
 * row p at pyr[0] + p * RC_REC_COUNT(W2) * RC_REC_BYTES, 16-byte aligned),
 * record r holding
 *     slots  0..25   level-2 elements 4r - 14 .. 4r + 11,
 *     slots 26..63   level-0 elements 16r - 26 .. 16r + 11
 * (zeros outside the level's width), so a pixel whose floor(x/2) lies in
 * [8r - 8, 8r) reads every tap of all four levels (radius <= 4) from record
 * r.  The values are the row layout's bit for bit, and so are the lookups.
 * rc_corr_build: bf16 fmaps and pyramid, nbuf 3 with pyr[1] == pyr[2] ==
 * NULL (pyr_ld ignored), 64 < W2 <= 320, D > 224, no shadow copies;
 * rc_corr_lookup_chain / _step (chain != 0): RC_BF16, levels 4, radius 1..4,
 * pyr[0] the records and pyr[1..3] NULL, widths[0] = W2; channels-last output
 * allowed.  RC_EUNSUPPORTED otherwise; the other entry points refuse it.
 * A pixel row's records take RC_REC_COUNT(W2) * 128 bytes, against about
 * 2 * 2 * (W2 + W2 / 4) for the shadowed rows (2816 vs 1556 at W2 = 311):
 * the build writes more, and each lookup reads half the lines. */
#define RC_LAYOUT_RECORDS 0x100000
#define RC_REC_SLOTS 64
#define RC_REC_BYTES 128
#define RC_REC_COUNT(W2) (((((W2) >> 1) + 15) >> 3) + 1)

/* return codes */
#define RC_OK            0
#define RC_EINVAL        1  /* bad shape / pointer / alignment / parameter */
#define RC_EUNSUPPORTED  2  /* valid request this build does not implement */
#define RC_EHIP          3  /* HIP runtime error (launch / device) */

/* Maximum pyramid buffers one rc_corr_build call writes (num_levels + 1). */
#define RC_MAX_LEVELS 8

int rc_abi_version(void);
const char *rc_last_error(void);

/* Volume + pyramid (model.py:284-295, :318-326).
 *   fmap1: [B][D][H][W1], fmap2: [B][D][H][W2], contiguous, element type
 *          fmap_dtype (RC_F32, or RC_BF16 for the bf16 MFMA path, or RC_F16
 *          with an RC_F16 pyramid for the fp16 one).
 *   pyr[l], l < nbuf: device buffers of B*H*W1 rows of W2 >> l elements of
 *          pyr_dtype, row stride pyr_ld[l] elements (>= W2 >> l; NULL pyr_ld =
 *          dense rows).  Level 0 is the volume divided by sqrtf(D), level l+1
 *          the pairwise mean of level l along w2 (floor width).  The
 *          reference builds num_levels+1 buffers (model.py:293); pass
 *          nbuf = num_levels + 1.  Padding rows to a multiple of 16 bytes lets
 *          every store be a full aligned vector (the padding is written with
 *          don't-care values and never read).
 *   Requires (W2 >> (nbuf-1)) >= 1 (the reference raises otherwise) and
 *   16-byte aligned pointers.
 *   Arithmetic: fmap_dtype == pyr_dtype == RC_F32 runs the split-bf16 fp32
 *   kernel (ABI v6; see RC_BUILD_EXACT_F32, which selects the exact fp32 MFMA
 *   kernel v_mfma_f32_16x16x4_f32 instead).  Any bf16 operand (bf16 fmaps, or a
 *   bf16 pyramid requested for fp32 fmaps, which are rounded to bf16 on
 *   load) runs the bf16 MFMA kernel (v_mfma_f32_16x16x32_bf16, fp32
 *   accumulation); pooling is done on the fp32 accumulators either way.
 *   An RC_F16 pyramid (see RC_F16) runs the same kernels on
 *   v_mfma_f32_16x16x32_f16. */
int rc_corr_build(const void *fmap1, const void *fmap2, int fmap_dtype,
                  int B, int D, int H, int W1, int W2,
                  void *const *pyr, const long *pyr_ld, int nbuf, int pyr_dtype,
                  void *stream);

/* One pooling step (model.py:294): out[p][j] = (in[p][2j] + in[p][2j+1]) / 2,
 * j < W_in/2, for p < rows; row strides ld_in / ld_out elements.  dtype
 * RC_F32, RC_BF16 or RC_F16 (the 16-bit types round once). */
int rc_corr_pool(const void *in, long ld_in, void *out, long ld_out, long rows,
                 int W_in, int dtype, void *stream);

/* Lookup (model.py:297-316, :267-281).
 *   pyr[i], i < levels: B*H*W1 rows of widths[i] elements of pyr_dtype, row
 *          stride pyr_ld[i] elements (NULL = dense), 16-byte aligned base.
 *   coords_x: x channel of the (B,2,H,W1) fp32 coords, element (b,h,w) at
 *          coords_x[b*coord_batch_stride + h*W1 + w] (the y channel is
 *          ignored, model.py:299/:308).
 *   out:   [B][levels*(2*radius+1)][H][W1] fp32, channel = level*(2r+1)+(t+r).
 *   radius in 1..8, levels in 1..RC_MAX_LEVELS.
 *   A level of width 1 is accepted, here and by every entry point that
 *   samples a pyramid: the sampler normalises by widths[i] - 1 = 0
 *   (model.py:271), so every tap of that level is NaN at every x, finite or
 *   not, exactly as the reference's arithmetic gives (the tap weights are
 *   NaN, so the zero-padding short cuts for far-away x do not show).  The
 *   reference itself never looks such a level up: its pyramid has
 *   num_levels + 1 levels, so level num_levels - 1 is at least 2 wide. */
int rc_corr_lookup(const void *const *pyr, const int *widths, const long *pyr_ld,
                   int pyr_dtype, int levels, int radius, const float *coords_x,
                   long coord_batch_stride, int B, int H, int W1, float *out,
                   void *stream);

/* Lookup fused with the motion encoder's first conv (model.py:199, :206):
 *   out[b][c][h][w] = act(bias[c] + sum_k weight[c][k] * corr[b][k][h][w]),
 *   corr = the rc_corr_lookup result (k = level*(2r+1) + tap, never written),
 *   weight: [cout][levels*(2r+1)] fp32 (a 1x1 Conv2d weight), bias: [cout] or
 *   NULL, act = ReLU when relu != 0.  out: [B][cout][H][W1] fp32.
 *   levels 2..4, radius 1..4.  Reads every level (one window each): for the
 *   pair layout CorrBlock1D stores, and for an fp16 / bf16 output, see
 *   rc_corr_lookup_chain_conv. */
int rc_corr_lookup_conv(const void *const *pyr, const int *widths, const long *pyr_ld,
                        int pyr_dtype, int levels, int radius, const float *coords_x,
                        long coord_batch_stride, int B, int H, int W1,
                        const float *weight, const float *bias, int cout, int relu,
                        float *out, void *stream);

/* Backward of rc_corr_lookup_conv (ABI v12; autograd of model.py:199, :206
 * taken together with the lookup), for training with the fused layer.  With
 * corr and pre[c] = bias[c] + sum_k weight[c][k] * corr[k] recomputed from the
 * pyramid exactly as the forward computes them (same helpers, same summation
 * order, so the ReLU mask is the forward's bit for bit and nothing from the
 * forward is kept), and g[c] = grad_out[b][c][h][w] * (relu ? pre[c] > 0 : 1):
 *   grad_corr[b][k][h][w] = sum_c weight[c][k] * g[c]
 *                        [B][levels*(2r+1)][H][W1] fp32 contiguous: the
 *                        grad_out that rc_corr_lookup_backward and
 *                        rc_corr_lookup_backward_calls consume;
 *   grad_weight[c][k]   = sum over pixels of g[c] * corr[k],  [cout][levels*(2r+1)];
 *   grad_bias[c]        = sum over pixels of g[c],            [cout].
 *   All three are overwritten; each may be NULL and is then not computed (all
 *   NULL: RC_EINVAL).  grad_out: [B][cout][H][W1] fp32 contiguous.  pyr ..
 *   relu: rc_corr_lookup_conv's arguments, with its checks, flag refusals and
 *   RC_EUNSUPPORTED cases (levels 2..4, radius 1..4; fp32 or bf16 pyramid).
 *   workspace: RC_LOOKUP_CONV_BWD_WS(B*H*W1, cout, levels*(2r+1)) floats
 *   holding one partial sum per workgroup of 256 pixels between the two
 *   launches; required exactly when grad_weight or grad_bias is given (with
 *   both NULL there is one launch).  B*H*W1 == 0 writes zeros to grad_weight
 *   and grad_bias.  No atomics: every sum has a fixed order, so results repeat
 *   bit for bit. */
#define RC_LOOKUP_CONV_BWD_WS(P, cout, cin) \
    ((((long long)(P) + 255) / 256) * (long long)(cout) * ((cin) + 1))   /* floats */
int rc_corr_lookup_conv_backward(const void *const *pyr, const int *widths, const long *pyr_ld,
                                 int pyr_dtype, int levels, int radius, const float *coords_x,
                                 long coord_batch_stride, int B, int H, int W1,
                                 const float *weight, const float *bias, int cout, int relu,
                                 const float *grad_out, float *grad_corr, float *grad_weight,
                                 float *grad_bias, float *workspace, void *stream);

/* rc_corr_lookup_conv on the pair layout (added within ABI v13): the lookup
 * half is rc_corr_lookup_chain's pair kernel -- levels 0 and 2 read (each
 * pixel's span from the RC_SHADOW copy that touches fewer lines, where
 * given), levels 1 and 3 derived in registers -- and the conv half is
 * rc_corr_lookup_conv's chain (bias, one fmaf per k ascending, ReLU), so with
 * an fp32 `out` the result equals rc_corr_lookup_conv's on the full pyramid
 * bit for bit, at ~2.8 instead of ~4.4 128-B lines read per pixel and with
 * levels 1 and 3 never in memory.
 *   Layout: pair only -- levels == 2, or levels == 4 with pyr[2] != NULL;
 *   pyr[1] and pyr[3] may be NULL and are never read.  RC_F32 or RC_BF16,
 *   RC_SHADOW / RC_SHADOW_LEVEL(l) honoured as by the pair kernel.  Checks
 *   are rc_corr_lookup_chain's (widths[i] == widths[i-1] / 2, level-0 width
 *   <= 65536, radius 1..4, 16-byte aligned levels, row strides whole 16-B
 *   chunks).
 *   out: [B][cout][H][W1] fp32, or IEEE fp16 / bfloat16 with RC_OUT_F16 /
 *   RC_OUT_BF16: each element the fp32 result rounded once to nearest even
 *   (Tensor.to(dtype) of the fp32 output bit for bit; conventions as for
 *   rc_corr_lookup_chain).  Both flags: RC_EINVAL.
 *   RC_EUNSUPPORTED, with a message, before any launch and whatever B is:
 *   RC_OUT_CHANNELS_LAST, RC_LAYOUT_RECORDS, RC_LAYOUT_DISPARITY, 3 levels,
 *   4 levels without level 2.  cout < 1 and a null weight (with B*H*W1 > 0)
 *   are RC_EINVAL; B*H*W1 == 0 is RC_OK. */
int rc_corr_lookup_chain_conv(const void *const *pyr, const int *widths, const long *pyr_ld,
                              int pyr_dtype, int levels, int radius, const float *coords_x,
                              long coord_batch_stride, int B, int H, int W1,
                              const float *weight, const float *bias, int cout, int relu,
                              void *out, void *stream);

/* Backward of rc_corr_lookup_chain_conv (added within ABI v13):
 * rc_corr_lookup_conv_backward with the correlation recomputed from the pair
 * layout.  Arguments, NULL combinations, workspace
 * (RC_LOOKUP_CONV_BWD_WS, the same layout; the second launch is the same
 * reduction) and the B*H*W1 == 0 behaviour are rc_corr_lookup_conv_backward's;
 * layout, checks and refusals are rc_corr_lookup_chain_conv's.  grad_out and
 * the three gradients are fp32: RC_OUT_F16 / RC_OUT_BF16 are RC_EUNSUPPORTED
 * (a half-precision forward output is the rounded fp32 one; widen its
 * gradient).  With the same correlation bits, the same 256 pixels per
 * workgroup and the same summation order, all three gradients equal
 * rc_corr_lookup_conv_backward's on the full pyramid bit for bit. */
int rc_corr_lookup_chain_conv_backward(const void *const *pyr, const int *widths, const long *pyr_ld,
                                       int pyr_dtype, int levels, int radius, const float *coords_x,
                                       long coord_batch_stride, int B, int H, int W1,
                                       const float *weight, const float *bias, int cout, int relu,
                                       const float *grad_out, float *grad_corr, float *grad_weight,
                                       float *grad_bias, float *workspace, void *stream);

/* Lookup over a pool-chain fp32 pyramid (what rc_corr_build writes), same
 * arguments and bit-identical results as rc_corr_lookup with RC_F32, but
 * some levels are recomputed from others (level l+1 = pairwise mean of level
 * l, the fp32 ops of model.py:294) instead of read.  pyr[i], i >= 1, may be
 * NULL (not stored); the kernel is chosen from what is given:
 *   levels 2, or levels 4 with pyr[2] != NULL: the pair kernel reads levels 0
 *     and 2 (one span of each serves two levels); level-0 width <= 65536;
 *   otherwise levels 3..4 with pyr[1] != NULL: the level-1 chain kernel reads
 *     levels 0 and 1 (one level-1 span serves levels 1..L-1).
 * Requires widths[i] == widths[i-1] / 2, the read levels' row strides whole
 * 16-B chunks, radius 1..4.  Levels given but not read must still hold the
 * pool chain for the results to equal rc_corr_lookup's.  pyr_dtype RC_BF16
 * (pair layout only): every level is the bf16-rounded pool of the level below
 * as stored -- what rc_corr_build and rc_corr_pool write for a bf16 pyramid,
 * and what avg_pool2d gives on bf16 tensors.  (ABI v4 added pyr_dtype.)
 * out: fp32, or the element type RC_OUT_F16 / RC_OUT_BF16 asks for (ABI v13). */
int rc_corr_lookup_chain(const void *const *pyr, const int *widths, const long *pyr_ld,
                         int pyr_dtype, int levels, int radius, const float *coords_x,
                         long coord_batch_stride, int B, int H, int W1, void *out,
                         void *stream);

/* One iteration of the forward loop's corr step in one launch: the
 * coordinate update that ends the previous iteration (coords1 + delta_flow
 * with delta_flow[:,1] = 0, the loop tail SURVEY Appendix A D8), then
 * flow = coords1 - coords0 (model.py:377, coords0 = coords_grid :329-332),
 * then the lookup at the new coords1 (:376).  coords1, delta, coords1_out,
 * flow_out: (B,2,H,W1) fp32 contiguous; delta NULL = no update (first
 * iteration); coords1_out may alias coords1.  chain != 0 runs
 * rc_corr_lookup_chain's kernel (its preconditions apply), else
 * rc_corr_lookup's.  The lookup output is bit-identical to theirs at the
 * updated coordinates; coords1_out and flow_out are bit-identical to the
 * PyTorch ops they replace.  SURVEY.md §8f rank 4.  out: fp32, or (chain != 0,
 * pair or records kernel) the element type RC_OUT_F16 / RC_OUT_BF16 asks for. */
int rc_corr_lookup_step(const void *const *pyr, const int *widths, const long *pyr_ld,
                        int pyr_dtype, int levels, int radius, int chain,
                        const float *coords1, const float *delta, float *coords1_out,
                        float *flow_out, int B, int H, int W1, void *out, void *stream);

/* Backward of rc_corr_lookup (model.py:297-316 through grid_sample's input
 * gradient, :275): for every pixel p, level i and tap t, adds
 * (x0+1-x')*g to grad_pyr[i][p][x0] and (x'-x0)*g to grad_pyr[i][p][x0+1]
 * (zero-padded taps add nothing), g = grad_out[b][i*(2r+1)+t][h][w].
 *   grad_pyr[i]: fp32, B*H*W1 rows of widths[i], row stride grad_ld[i]
 *          (multiple of 4; NULL grad_ld = dense, then widths must be
 *          multiples of 4), 16-byte aligned.  Accumulates: zero the buffers
 *          once, then call once per lookup call.
 *   grad_out: [B][levels*(2r+1)][H][W1] fp32 contiguous.  Other arguments as
 *          rc_corr_lookup.  No atomics: pixel p owns row p.
 *   Pair layout: with levels 2 or 4, grad_pyr[1] (and grad_pyr[3]) NULL and
 *          radius <= 4, the gradients of levels 1 and 3 are added, already
 *          through avg_pool2d's backward (/2 to both children), to levels 0
 *          and 2; pass such buffers to rc_corr_build_backward with levels = 3
 *          and grad_pyr[1] = NULL.
 *   levels | RC_SHADOW_LEVEL(0) / RC_SHADOW_LEVEL(2) (4-level pair layout
 *          only, else RC_EUNSUPPORTED): the allocation of grad_pyr[l] also
 *          holds a zeroed copy at RC_SHADOW_OFFSET(B*H*W1, grad_ld[l], 4)
 *          bytes; each pixel's span goes to the copy in which it touches
 *          fewer 128-B lines.  Pass the same bits to rc_corr_build_backward,
 *          which sums the copies.  Measured not to pay at config 2
 *          (DESIGN.md §3.4b); off by default. */
int rc_corr_lookup_backward(void *const *grad_pyr, const int *widths, const long *grad_ld,
                            int levels, int radius, const float *coords_x,
                            long coord_batch_stride, int B, int H, int W1,
                            const float *grad_out, void *stream);

/* The gradients of n_calls lookups into the same gradient buffers, summed in
 * one pass (ABI v7; model.py:376 runs the lookup `iters` times, and autograd
 * adds every call's grid_sample input gradient, :275, into the levels):
 * equal to n_calls rc_corr_lookup_backward calls up to the association of
 * the fp32 sums.  coords_x[c], coord_batch_stride[c], grad_out[c]: call c's
 * arguments as in rc_corr_lookup_backward (all calls share B, H, W1, levels,
 * radius).  levels | RC_GRAD_OVERWRITE: the buffers receive the sum instead
 * of having it added (they need not be zeroed first; row padding up to the
 * next multiple of 4 columns is written as zeros).  With the pair layout each
 * lane keeps the union of its calls' windows of its pixel's rows on chip
 * (compact rows: any level-0 width whose LDS budget max(5120, 2(W + 8r + 24))
 * floats fits 64 KB, i.e. W up to about 8K), so each call's inputs are read
 * once and each row written once, in launches of up to 32
 * calls.  Wider rows, per-call coords or grad_out extents past the kernel's
 * 32-bit offsets, and the per-level layout run a loop over
 * rc_corr_lookup_backward instead -- chosen for the whole request before the
 * first launch.  RC_SHADOW_LEVEL bits are RC_EUNSUPPORTED here; other flag
 * bits than RC_GRAD_OVERWRITE are RC_EINVAL.  RC_GRAD_OVERWRITE with
 * n_calls == 0 is RC_EINVAL; n_calls == 0 otherwise does nothing. */
#define RC_GRAD_OVERWRITE 0x40000
int rc_corr_lookup_backward_calls(void *const *grad_pyr, const int *widths, const long *grad_ld,
                                  int levels, int radius, int n_calls,
                                  const float *const *coords_x, const long *coord_batch_stride,
                                  int B, int H, int W1, const float *const *grad_out,
                                  void *stream);

/* Backward of rc_corr_build (model.py:284-295 pooling, :318-326 volume):
 *   Dl_{L-1} = grad_pyr[L-1], Dl_i[k] = grad_pyr[i][k] + Dl_{i+1}[k/2] / 2
 *   (avg_pool2d's backward, floor widths), G = Dl_0 / sqrtf(D), and
 *   grad_fmap1[b][d][h][w1] = sum_w2 G[b,h,w1,w2] * fmap2[b][d][h][w2]
 *   grad_fmap2[b][d][h][w2] = sum_w1 G[b,h,w1,w2] * fmap1[b][d][h][w1]
 *   (overwritten, fp32).  grad_pyr[l], l < levels: fp32 B*H*W1 rows of
 *   W2 >> l, row stride grad_ld[l] (grad_ld[0] % 4 == 0).  fmap_dtype RC_F32
 *   only.  When B*H*W1 == 0 nothing is written.
 *   ABI v8: the two GEMMs run on bf16 MFMA with every fp32 operand split
 *   exactly into three bf16 pieces (six products per fp32 product, fp32
 *   accuracy, as rc_corr_build's default) when W1 % 4 == W2 % 4 == 0 and the
 *   gradients are pair-folded or 1-2 levels; otherwise, or with
 *   fmap_dtype | RC_BUILD_EXACT_F32 (needed only for non-finite values), on
 *   exact fp32 MFMA.
 *   levels == 3 with grad_pyr[1] == NULL: pair-folded gradients from
 *   rc_corr_lookup_backward's pair layout, Dl_0[k] = g_0[k] + g_2[k>>2] / 4;
 *   with levels | RC_SHADOW_LEVEL(0) / (2) each g_l is primary + shadow copy. */
int rc_corr_build_backward(const void *fmap1, const void *fmap2, int fmap_dtype,
                           int B, int D, int H, int W1, int W2,
                           const void *const *grad_pyr, const long *grad_ld, int levels,
                           float *grad_fmap1, float *grad_fmap2, void *stream);

/* Convex upsampling with the update block's mask
 * (model.py:238-241, 0.25-scaled at :264; f = 2^n_downsample, :236):
 *   out[n][c][f h + i][f w + j] = sum_k softmax_k(mask[n][k f^2 + i f + j][h][w])
 *                                 * f * flow[n][c][h + dy_k][w + dx_k]
 *   k = 3 (dy+1) + (dx+1), zeros outside the image (RAFT-Stereo's upsampler,
 *   F.unfold + softmax; the reference builds the mask but never applies it).
 *   flow (N,C,H,W), mask (N,9f^2,H,W), out (N,C,fH,fW): fp32 contiguous;
 *   out aligned to min(16, 4 f) bytes (else RC_EINVAL).  factor 1, 2, 4 or 8.
 *   Non-finite masks follow the softmax: a -inf tap has weight 0 while another
 *   tap of its sub-pixel is finite; a sub-pixel whose nine taps are all -inf,
 *   or that holds +inf or NaN, gives NaN in its output element. */
int rc_convex_upsample(const float *flow, const float *mask, int N, int C, int H, int W,
                       int factor, float *out, void *stream);

/* Backward of rc_convex_upsample (ABI v11), for a loss taken on the
 * full-resolution prediction.  With wt = the forward's softmax weights
 * (recomputed from mask; nothing else is kept from the forward),
 * nb[c][k] = f * flow[n][c][h + dy_k][w + dx_k] and g = grad_out:
 *   grad_mask[n][k f^2 + i f + j][h][w] = wt_k * (d_k - sum_k' wt_k' d_k'),
 *                        d_k = sum_c g[n][c][f h + i][f w + j] * nb[c][k]
 *   grad_flow[n][c][y][x] = sum_k P[n][c][k][y - dy_k][x - dx_k],
 *                        P[n][c][k][h][w] = f * sum_{i,j} wt_k * g[n][c][f h + i][f w + j]
 *   (taps whose source pixel lies outside the image dropped).
 *   flow, mask, grad_out: fp32 contiguous, the shapes of rc_convex_upsample's
 *   flow, mask and out; grad_out aligned to min(16, 4 f) bytes.  grad_flow
 *   (N,C,H,W) and grad_mask (N,9f^2,H,W) are overwritten; either may be NULL
 *   and is then not computed (both NULL: RC_EINVAL).  workspace:
 *   RC_UPSAMPLE_BWD_WS(N, C, H, W) floats holding P between the two launches,
 *   required exactly when grad_flow != NULL.  factor 1, 2, 4 or 8.  No
 *   atomics: every sum has a fixed order, so results repeat bit for bit. */
#define RC_UPSAMPLE_BWD_WS(N, C, H, W) ((long long)(N) * (C) * 9 * (H) * (W))   /* floats */
int rc_convex_upsample_backward(const float *flow, const float *mask, const float *grad_out,
                                int N, int C, int H, int W, int factor,
                                float *grad_flow, float *grad_mask, float *workspace, void *stream);

/* The upsampling head of an inference forward (added within ABI v13,
 * additive: a caller that needs it checks for the symbol): rc_convex_upsample
 * on the mask as the update block's last convolution wrote it,
 *   out[n][c][f h + i][f w + j] = sum_k softmax_k(scale * mask[n][k f^2 + i f + j][h][w])
 *                                 * f * flow[n][c][h + dy_k][w + dx_k].
 *   mask: (N, 9 f^2, H, W) elements of mask_dtype (RC_F32, RC_F16 or RC_BF16),
 *   addressed by mask_strides[0..2] = its (batch, channel, pixel) strides in
 *   elements, pixel = h W + w.  Two layout classes: planar (pixel stride 1,
 *   channel stride H W: NCHW, any batch stride) and interleaved (channel
 *   stride 1, pixel stride 9 f^2: channels-last, any batch stride); a stride
 *   along an axis of length 1 is ignored; anything else is RC_EUNSUPPORTED.
 *   scale: applied in fp32 to the widened logit, rounded once.  0.25 is the
 *   update block's factor (model.py:264); 1.0 gives rc_convex_upsample.
 *   flow: fp32, pixel stride 1, flow_strides[0..1] = its (batch, channel)
 *   strides in elements: the x-channel of an (N, 2, H, W) tensor passes as it
 *   is.  out: fp32 contiguous (N, C, f H, f W), aligned to min(16, 4 f) bytes.
 *   The result equals rc_convex_upsample on the fp32 contiguous mask
 *   scale * (float)mask bit for bit (the same arithmetic, in the same order),
 *   in both classes and at every access width: mask loads are 8 bytes per lane
 *   (planar) or f elements per lane (interleaved) where the base, the batch
 *   stride and H W allow, one element otherwise.  Non-finite logits behave as
 *   rc_convex_upsample's.
 *   RC_EINVAL: an unknown mask_dtype, N < 0, C < 1, H < 0, W < 0, a factor
 *   other than 1, 2, 4, 8, a null stride array, a negative stride and, with
 *   N*H*W > 0, a null pointer, flow or mask not aligned to its element, out
 *   not aligned.  N*H*W == 0: RC_OK, nothing launched.  All checks run before
 *   the launch. */
int rc_upsample_head(const float *flow, const long *flow_strides, const void *mask,
                     const long *mask_strides, int mask_dtype, float scale, int N, int C, int H, int W,
                     int factor, float *out, void *stream);

/* The elementwise glue of the ConvGRU update between its convolutions (added
 * within ABI v13), two memory-bound launches:
 *   rc_gru_gates:  z_out  = sigmoid(z_pre + cz)
 *                  rh_out = sigmoid(r_pre + cr) * h
 *   rc_gru_blend:  h_out  = (1 - z) * h + z * tanh(q_pre + cq)
 *   Operands: N x C x HW arrays of one element type `dtype` (RC_F32, RC_F16 or
 *   RC_BF16), operand k addressed by strides[3k .. 3k+2] = its (batch,
 *   channel, pixel) strides in elements, in the order of the pointer
 *   arguments (7 triples for gates, 5 for blend).  One call therefore takes
 *   dense NCHW tensors, channel slices of a larger buffer (the two halves of
 *   a stacked z/r convolution output; the first C channels of the [r*h, x]
 *   convolution input, whose other channels are not touched) and
 *   channels-last tensors.  All operands of a call are of one layout class:
 *   planar (every pixel stride 1) or interleaved (every channel stride 1); a
 *   stride along an axis of length 1 is ignored.  Any other mix is
 *   RC_EUNSUPPORTED, whatever N is.  Accesses are 16 bytes per lane where
 *   every base address and stride and the unit-stride length allow, else 8,
 *   else one element; all paths give the same bits.
 *   Arithmetic: fp32 on the widened inputs, every operation of the
 *   expressions above rounded on its own, one rounding to nearest even at
 *   the store: an fp16 / bf16 result is Tensor.to(dtype) of the fp32 result on
 *   the widened inputs, bit for bit.  sigmoid is 0 / 1 and tanh -1 / +1
 *   exactly at +-inf and wherever they saturate (never NaN); NaN in, NaN out.
 *   Aliasing: z_out may be z_pre and h_out may be h (exactly, same strides);
 *   rh_out must not be h (RC_EINVAL); no other overlap between an output and
 *   an operand.
 *   RC_EINVAL: an unknown dtype, C < 1, N < 0, HW < 0, a null stride array, a
 *   negative stride and, with N*HW > 0, a null operand or one not aligned to
 *   its element size.  N*HW == 0: RC_OK, nothing launched.  N*C*HW >= 2^32:
 *   RC_EUNSUPPORTED.  All checks run before the launch. */
int rc_gru_gates(const void *z_pre, const void *r_pre, const void *cz, const void *cr, const void *h,
                 void *z_out, void *rh_out, const long *strides, int dtype, int N, int C, long HW,
                 void *stream);
int rc_gru_blend(const void *z, const void *q_pre, const void *cq, const void *h, void *h_out,
                 const long *strides, int dtype, int N, int C, long HW, void *stream);

/* Backward of rc_gru_gates / rc_gru_blend (added within ABI v13, additive like
 * the two above: a caller that needs them checks for the symbols), for
 * training with the fused update block; one launch each.  With the incoming
 * gradients g_out (of h_out), g_z (of z_out) and g_rh (of rh_out):
 *   rc_gru_blend_backward:  q      = tanh(q_pre + cq)
 *                           g_z    = g_out * (q - h)
 *                           g_qpre = (g_out * z) * (1 - q*q)     also cq's gradient
 *                           g_h    = g_out * (1 - z)
 *   rc_gru_gates_backward:  r      = sigmoid(r_pre + cr)
 *                           g_zpre = g_z * ((1 - z) * z)         also cz's gradient
 *                           g_rpre = (g_rh * h) * ((1 - r) * r)  also cr's gradient
 *                           g_h    = g_rh * r
 *   z is the forward's output; r and q are recomputed from the pre-activations
 *   exactly as the forward computes them, so nothing else is kept.  Each g_h
 *   is that kernel's contribution to h's gradient; the caller adds them.
 *   Operands, strides (9 triples for gates, 8 for blend, in pointer order),
 *   layout classes, access widths, arithmetic (fp32 on the widened inputs,
 *   every operation above rounded on its own, one rounding at the store) and
 *   the RC_EINVAL / RC_EUNSUPPORTED / RC_OK cases are rc_gru_gates'.  Where
 *   the forward saturates (sigmoid 0 / 1, tanh +-1) g_zpre, g_rpre and g_qpre
 *   are +-0 for finite incoming gradients; NaN in, NaN out.
 *   Aliasing: an output may be an input (exactly, same strides: g_zpre over
 *   g_z, g_h over g_out); two outputs in one array are RC_EINVAL.  g_zpre and
 *   g_rpre are normally the channel halves of one (N, 2C) buffer, the
 *   gradient of the stacked z/r convolution's output. */
int rc_gru_gates_backward(const void *g_z, const void *g_rh, const void *z, const void *r_pre, const void *cr,
                          const void *h, void *g_zpre, void *g_rpre, void *g_h,
                          const long *strides, int dtype, int N, int C, long HW, void *stream);
int rc_gru_blend_backward(const void *g_out, const void *z, const void *q_pre, const void *cq, const void *h,
                          void *g_z, void *g_qpre, void *g_h,
                          const long *strides, int dtype, int N, int C, long HW, void *stream);

/* The input assembly of a ConvGRU update (added within ABI v13, additive): the
 * N x (sum of channels) x H x W buffer `dst` -- [h, x], or a channel slice of
 * it -- filled by ONE launch from nparts sources.  Part i fills the next
 * channels[i] channels of dst from src[i], an N x channels[i] x src_h[i] x
 * src_w[i] array of element type src_dtype[i] with the element strides
 * src_strides[4i .. 4i+3] (batch, channel, row, column), by mode[i]:
 *   RC_PART_COPY      dst = (T)src; src_h x src_w is H x W.  Same type: the
 *                     same bits for every non-NaN value.
 *   RC_PART_POOL2X    F.avg_pool2d(src, 3, stride=2, padding=1): the sum of
 *                     the window's in-image taps row by row from 0.0f, then a
 *                     correctly rounded division by 9.0f (the padding is
 *                     counted).  H = (src_h - 1) / 2 + 1, W likewise.
 *   RC_PART_BILINEAR  F.interpolate(src, (H, W), mode="bilinear",
 *                     align_corners=True), ATen's sequence: per axis with
 *                     source size S and destination size D, scale = D > 1 ?
 *                     (float)(S-1) / (float)(D-1) : 0, s = scale * i, i0 =
 *                     (int)s, i1 = i0 + (i0 < S-1), l1 = s - i0, l0 = 1 - l1;
 *                     l0h*(l0w*a + l1w*b) + l1h*(l0w*c + l1w*d).  Any src_h,
 *                     src_w >= 1; the same size gives the source's values.
 *   Arithmetic as for rc_gru_gates: fp32 on the widened inputs, every
 *   operation rounded on its own, one rounding to dst_dtype at the store; the
 *   same bits whatever the layouts and access widths.
 *   dst: element type dst_dtype, strides dst_strides[0..3]; planar (column
 *   stride 1 and row stride W) or interleaved (channel stride 1), anything
 *   else is RC_EUNSUPPORTED.  The sources take any non-negative strides and
 *   any of the three element types, each independently of dst.  Accesses are
 *   16 bytes of dst per lane where every base, stride and length allows (an
 *   interleaved dst: sources of channel stride 1 and channel counts that are
 *   whole vectors; a planar one: W a whole number of vectors and copied
 *   sources of column stride 1), else 8 bytes, else one element.
 *   RC_EINVAL, naming the argument, before any launch: nparts outside
 *   1..RC_GRU_MAX_PARTS, a null pointer (arrays, dst, src[i]), an unknown
 *   dst_dtype / src_dtype[i] / mode[i], channels[i] < 1, src_h[i] or src_w[i]
 *   < 1, a negative size or stride, a copied or pooled part whose size does
 *   not give H x W, dst == src[i] (no operand may overlap dst), and with work
 *   to do a pointer not aligned to its element size.  N, H or W == 0: RC_OK,
 *   nothing launched.  More than 2^31 - 1 elements of dst: RC_EUNSUPPORTED.
 *   All offsets are computed in 64 bits. */
#define RC_GRU_MAX_PARTS 4
#define RC_PART_COPY     0
#define RC_PART_POOL2X   1
#define RC_PART_BILINEAR 2
int rc_gru_assemble(void *dst, const long *dst_strides, int dst_dtype, int N, int H, int W, int nparts,
                    const void *const *src, const long *src_strides, const int *src_dtype, const int *mode,
                    const int *channels, const int *src_h, const int *src_w, void *stream);

/* The adjoint of rc_gru_assemble (added within ABI v13, additive): from the
 * gradient of the assembled N x (sum of channels) x H x W buffer, the gradient
 * of every part's source, ONE launch.
 *   g: the gradient of the buffer, element type g_dtype, strides g_strides[0..3];
 *   planar or interleaved exactly as dst of rc_gru_assemble, anything else is
 *   RC_EUNSUPPORTED.  g2: NULL, or a second gradient of the same shape, strides
 *   and type: part channels c >= g2_c0 then use G = g + g2, added in fp32 after
 *   widening, the others G = g; g2 is never read below channel g2_c0 (one
 *   launch for the gradients of [h, x] and of [r*h, x], whose first channels
 *   belong to different tensors).
 *   grad_src[i] receives the gradient of part i's source: N x channels[i] x
 *   src_h[i] x src_w[i] elements of type grad_dtype[i] with the element strides
 *   grad_strides[4i .. 4i+3], any non-negative ones.  NULL skips the part; its
 *   channels still count, and its other entries are still checked.  Every
 *   element of every other output is written: a source pixel that no
 *   destination pixel reads (most pixels of a bilinear downscale) gets +0.
 *   No atomics: each lane owns the elements it stores and every sum has a fixed
 *   order, so the results repeat bit for bit and are the same whatever the
 *   layouts and access widths.  Arithmetic as for rc_gru_assemble: fp32 on the
 *   widened inputs, every operation rounded on its own, one rounding to
 *   grad_dtype[i] at the store.  By mode[i]:
 *   RC_PART_COPY      grad = (S)G.
 *   RC_PART_POOL2X    source pixel (y, x) sums G over the windows that contain
 *                     it: along H oy = y / 2 for even y, (y - 1) / 2 and
 *                     (y + 1) / 2 for odd y, only oy < H; W likewise.  The sum
 *                     is row-major from 0.0f, then one correctly rounded
 *                     division by 9.0f.
 *   RC_PART_BILINEAR  per axis the weight of destination index d on source
 *                     index s is (i0(d) == s ? l0(d) : 0) + (i1(d) == s ? l1(d)
 *                     : 0) with i0, i1, l0, l1 of rc_gru_assemble (where i1 ==
 *                     i0 both terms land on the same pixel); grad = sum_dy
 *                     wy(dy) * (sum_dx wx(dx) * G[dy][dx]), both sums ascending
 *                     from 0.0f over the destinations with i0 in {s - 1, s}.
 *                     Any sizes the forward accepts: a downscale, src_h or
 *                     src_w == 1 and H or W == 1 (scale 0) included.
 *   A unit of work is 16 bytes of g's element type along the unit-stride axis
 *   of g's layout class, of one output, where every base, stride and length
 *   allows (interleaved: outputs of channel stride 1, channel counts, channel
 *   offsets and g2_c0 that are whole vectors; planar: outputs of column stride
 *   1 and src_w a whole number of vectors), else 8 bytes, else one element;
 *   outputs of the other layout class take the one-element path.
 *   RC_EINVAL, naming the argument, before any launch: what rc_gru_assemble
 *   refuses (g for dst, grad_src / grad_strides / grad_dtype for src /
 *   src_strides / src_dtype; a NULL grad_src[i] is a skipped part), g2_c0
 *   outside 0 .. sum of channels, an output that is g, g2 or another output (no
 *   output may overlap a gradient or another output; equal base pointers are
 *   caught), g2 == g, every grad_src[i] NULL.  RC_EUNSUPPORTED: g neither
 *   planar nor interleaved; more than 2^31 - 1 elements in g or in an output.
 *   N, H or W == 0: RC_OK, nothing launched.  All offsets are computed in 64
 *   bits. */
int rc_gru_assemble_backward(const void *g, const void *g2, int g2_c0, const long *g_strides, int g_dtype,
                             int N, int H, int W, int nparts, void *const *grad_src, const long *grad_strides,
                             const int *grad_dtype, const int *mode, const int *channels, const int *src_h,
                             const int *src_w, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* RAFTCORR_H */
