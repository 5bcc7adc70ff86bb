// C-ABI entry points declared in include/raftcorr.h.
//
// Validation mirrors the reference's failure modes where it has them
// (e.g. W2 < 2^num_levels makes avg_pool2d raise at model.py:294), then
// launches on the caller's stream.  Nothing here allocates or synchronises, so
// every entry point is safe inside hipStreamBeginCapture.
// The helpers of all come first, then one section per family, its own helpers
// in front.  The order of the checks is part of the contract: callers rely on
// which refusal wins, and on every refusal coming before the empty-problem RC_OK.
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdint>
#include <cstdlib>

#include "../../include/raftcorr.h"
#include "common.h"

namespace {
thread_local char g_err[512] = "";

int fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}

int hip_rc(hipError_t e, const char *who, const char *what) {
    if (e == hipSuccess) return RC_OK;
    return fail(RC_EHIP, "%s: %s: %s", who, what, hipGetErrorString(e));
}

hipStream_t hip_stream(void *stream) { return reinterpret_cast<hipStream_t>(stream); }

// the element types are the kernels' element kinds (common.h)
static_assert(RC_F32 == rc::kF32 && RC_BF16 == rc::kBF16 && RC_F16 == rc::kF16, "element kinds");
bool known_kind(int dt) { return dt == RC_F32 || dt == RC_BF16 || dt == RC_F16; }
int elem_size(int dt) { return dt != RC_F32 ? 2 : 4; }

bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
bool elem_aligned(const void *p, int dt) { return reinterpret_cast<uintptr_t>(p) % (uintptr_t)elem_size(dt) == 0; }

// RC_SHADOW (ABI v5): byte offset from a stored level's base to its copy.
long long shadow_offset(long long rows, long long ld, int esize) { return RC_SHADOW_OFFSET(rows, ld, esize); }
// the RC_SHADOW_LEVEL bits of a flag word (pyr_dtype, or levels in the backward entry points): bit l = level l
unsigned shadow_mask(int word) { return ((unsigned)word >> 8) & 0xFFu; }

constexpr int RC_OUT_HALF = RC_OUT_F16 | RC_OUT_BF16;

// A pyr_dtype word, decoded once by check_flags.
struct Flags {
    int kind;           // the element type (low byte)
    unsigned shmask;    // RC_SHADOW_LEVEL bits
    bool cl;            // RC_OUT_CHANNELS_LAST
    bool disp, rec;     // RC_LAYOUT_DISPARITY: rows of W1 (or more) per diagonal; RC_LAYOUT_RECORDS: pyr[0] = the records
    bool exact;         // RC_BUILD_EXACT_F32
    int out_dt;         // LookupArgs::out_dt: 1 = RC_OUT_F16, 2 = RC_OUT_BF16, 0 = fp32
};
Flags decode_flags(int w) {
    return Flags{w & 0xFF, shadow_mask(w), (w & RC_OUT_CHANNELS_LAST) != 0, (w & RC_LAYOUT_DISPARITY) != 0,
                 (w & RC_LAYOUT_RECORDS) != 0, (w & RC_BUILD_EXACT_F32) != 0,
                 (w & RC_OUT_F16) ? 1 : (w & RC_OUT_BF16) ? 2 : 0};
}

// pyr_dtype bits an entry point accepts: the element type (low byte) and the
// RC_SHADOW_LEVEL bits always, and the RC_* flags of `accept`.  Decodes an
// accepted word into `f`.
int check_flags(const char *who, int pyr_dtype, int accept, Flags &f) {
    const unsigned known = 0xFFu | RC_SHADOW | (unsigned)accept;
    const int refused = pyr_dtype & ~accept;
    if (refused & RC_OUT_CHANNELS_LAST)
        return fail(RC_EUNSUPPORTED, "%s: RC_OUT_CHANNELS_LAST is only defined for "
                    "rc_corr_lookup_chain / rc_corr_lookup_step", who);
    if (refused & RC_OUT_HALF)
        return fail(RC_EUNSUPPORTED, "%s: RC_OUT_F16 / RC_OUT_BF16 are only defined for "
                    "rc_corr_lookup_chain / rc_corr_lookup_step", who);
    if ((pyr_dtype & RC_OUT_HALF) == RC_OUT_HALF)
        return fail(RC_EINVAL, "%s: RC_OUT_F16 and RC_OUT_BF16 exclude each other", who);
    if (refused & RC_LAYOUT_DISPARITY)
        return fail(RC_EUNSUPPORTED, "%s: RC_LAYOUT_DISPARITY is only defined for "
                    "rc_corr_build / rc_corr_lookup_chain", who);
    if (refused & RC_LAYOUT_RECORDS)
        return fail(RC_EUNSUPPORTED, "%s: RC_LAYOUT_RECORDS is only defined for "
                    "rc_corr_build / rc_corr_lookup_chain / rc_corr_lookup_step", who);
    if ((pyr_dtype & RC_LAYOUT_DISPARITY) && (pyr_dtype & RC_LAYOUT_RECORDS))
        return fail(RC_EINVAL, "%s: RC_LAYOUT_DISPARITY and RC_LAYOUT_RECORDS exclude each other", who);
    if ((unsigned)pyr_dtype & ~known)
        return fail(RC_EINVAL, "%s: unknown pyr_dtype flag bits 0x%x", who, (unsigned)pyr_dtype & ~known);
    f = decode_flags(pyr_dtype);
    return RC_OK;
}

bool is_pow2_float(float v) {
    int e;
    return std::frexp(v, &e) == 0.5f;
}

// The volume's divisor, torch.sqrt(torch.tensor(D).float()) (:326), as BuildArgs
// and BuildBwdArgs carry it; the reciprocal is exact when sqrt(D) is a power of two.
template <class Args>
void set_sqrt_d(Args &a, int D) {
    a.sq = std::sqrt((float)D);
    a.pow2 = is_pow2_float(a.sq) ? 1 : 0;
    a.scale = 1.0f / a.sq;
}
}  // namespace

extern "C" int rc_abi_version(void) { return RC_ABI_VERSION; }

extern "C" const char *rc_last_error(void) { return g_err; }

// ---- build and pool ------------------------------------------------------------------------------------------------
extern "C" int rc_corr_build(const void *fmap1, const void *fmap2, int fmap_dtype, int B, int D,
                             int H, int W1, int W2, void *const *pyr, const long *pyr_ld, int nbuf,
                             int pyr_dtype, void *stream) {
    g_err[0] = 0;
    const char *who = "rc_corr_build";
    Flags f;
    if (int e = check_flags(who, pyr_dtype, RC_BUILD_EXACT_F32 | RC_LAYOUT_DISPARITY | RC_LAYOUT_RECORDS, f)) return e;
    if (B < 0 || D <= 0 || H < 0 || W1 < 0 || W2 <= 0)
        return fail(RC_EINVAL, "rc_corr_build: bad shape B=%d D=%d H=%d W1=%d W2=%d", B, D, H, W1, W2);

    if (nbuf < 1 || nbuf > RC_MAX_LEVELS)
        return fail(RC_EINVAL, "rc_corr_build: nbuf=%d outside 1..%d", nbuf, RC_MAX_LEVELS);
    if ((W2 >> (nbuf - 1)) < 1)
        return fail(RC_EINVAL,
                    "rc_corr_build: pyramid level %d of width %d would be empty "
                    "(avg_pool2d output size too small, model.py:294)",
                    nbuf - 1, W2);
    if (!known_kind(fmap_dtype)) return fail(RC_EINVAL, "rc_corr_build: unknown fmap dtype %d", fmap_dtype);
    if (!known_kind(f.kind)) return fail(RC_EINVAL, "rc_corr_build: unknown pyramid dtype %d", f.kind);
    if (fmap_dtype == RC_F16 || f.kind == RC_F16) {
        // RC_F16: an fp16 pyramid from fp16 fmaps, or from fp32 fmaps rounded on load
        if (f.kind == RC_F32)
            return fail(RC_EUNSUPPORTED, "rc_corr_build: fp16 fmaps with an fp32 pyramid: widen the fmaps, or "
                        "ask for an RC_F16 pyramid");
        if (fmap_dtype == RC_BF16 || f.kind == RC_BF16)
            return fail(RC_EUNSUPPORTED, "rc_corr_build: fp16 and bf16 do not mix (fmap dtype %d, pyramid "
                        "dtype %d): one MFMA operand type per build", fmap_dtype, f.kind);
        if (f.rec)
            return fail(RC_EUNSUPPORTED, "rc_corr_build: RC_LAYOUT_RECORDS holds bf16 elements; an RC_F16 "
                        "pyramid is stored in rows");
        if (f.disp)
            return fail(RC_EUNSUPPORTED, "rc_corr_build: RC_LAYOUT_DISPARITY holds fp32 elements; an RC_F16 "
                        "pyramid is stored in rows");
        if (f.exact)
            return fail(RC_EUNSUPPORTED, "rc_corr_build: RC_BUILD_EXACT_F32 selects the fp32 MFMA kernel; an "
                        "RC_F16 pyramid is built on the fp16 MFMA");
    }
    if (!pyr) return fail(RC_EINVAL, "rc_corr_build: null pyramid array");
    if (f.disp) {   // RC_LAYOUT_DISPARITY: the split build's pair layout only
        if (fmap_dtype != RC_F32 || f.kind != RC_F32 || f.exact || f.shmask)
            return fail(RC_EUNSUPPORTED, "rc_corr_build: RC_LAYOUT_DISPARITY needs fp32 fmaps and pyramid, "
                        "the split build and no shadow copies");
        if (!(nbuf == 1 || (nbuf == 3 && !pyr[1])))
            return fail(RC_EUNSUPPORTED, "rc_corr_build: RC_LAYOUT_DISPARITY stores the pair layout: "
                        "nbuf 1, or 3 with pyr[1] NULL");
        if (W1 % 4 || W2 % 4)
            return fail(RC_EUNSUPPORTED, "rc_corr_build: RC_LAYOUT_DISPARITY needs W1, W2 multiples of 4");
        if (!pyr_ld) return fail(RC_EINVAL, "rc_corr_build: RC_LAYOUT_DISPARITY needs pyr_ld");
        for (int l = 0; l < nbuf; l += 2) {
            if (pyr_ld[l] < W1 || pyr_ld[l] % 4)
                return fail(RC_EINVAL, "rc_corr_build: disparity-major row stride %ld of level %d must be "
                            ">= W1 = %d and a multiple of 4", pyr_ld[l], l, W1);
            if ((long long)B * H * RC_SHEAR_ROWS(W2, W1, l) * pyr_ld[l] * 4 >= 0xFFFFFF00LL)
                return fail(RC_EUNSUPPORTED, "rc_corr_build: disparity-major level %d exceeds 4 GiB", l);
        }
    }
    if (f.rec) {   // RC_LAYOUT_RECORDS: the bf16 ring build's deferred epilogue, one tile per row
        if (fmap_dtype != RC_BF16 || f.kind != RC_BF16 || f.exact || f.shmask)
            return fail(RC_EUNSUPPORTED, "rc_corr_build: RC_LAYOUT_RECORDS needs bf16 fmaps and pyramid "
                        "and no shadow copies");
        if (nbuf != 3 || pyr[1] || pyr[2])
            return fail(RC_EUNSUPPORTED, "rc_corr_build: RC_LAYOUT_RECORDS stores the 4-level pair layout: "
                        "nbuf 3 with pyr[0] the records and pyr[1], pyr[2] NULL");
        if (W2 <= 64 || W2 > 320 || D <= 224)
            return fail(RC_EUNSUPPORTED, "rc_corr_build: RC_LAYOUT_RECORDS needs 64 < W2 <= 320 and D > 224 "
                        "(W2=%d D=%d)", W2, D);
        if ((long long)D * H * (W1 > W2 ? W1 : W2) * 2 >= (1LL << 30))
            return fail(RC_EUNSUPPORTED, "rc_corr_build: RC_LAYOUT_RECORDS: fmap image over 1 GiB");
    }
    if ((long long)B * H * W1 == 0) return RC_OK;
    if (!fmap1 || !fmap2 || !aligned16(fmap1) || !aligned16(fmap2))
        return fail(RC_EINVAL, "rc_corr_build: feature maps must be non-null and 16-byte aligned");
    const int nfused = nbuf < 7 ? nbuf : 7;
    for (int l = 0; l < nbuf; ++l) {
        // a NULL level l >= 1 inside the fused epilogue is computed (the next
        // level needs it) but not stored; later levels are pooled from memory
        const bool may_skip = l >= 1 && l < nfused && (nbuf <= 7 || l < 6);
        if (!pyr[l] && may_skip) continue;
        if (!pyr[l] || !aligned16(pyr[l]))
            return fail(RC_EINVAL, "rc_corr_build: pyramid buffer %d null or not 16-byte aligned", l);
        if (!f.disp && !f.rec && pyr_ld && pyr_ld[l] < (long)(W2 >> l))
            return fail(RC_EINVAL, "rc_corr_build: row stride %ld of level %d < width %d", pyr_ld[l],
                        l, W2 >> l);
    }

    rc::BuildArgs a{};
    a.f1 = fmap1;
    a.f2 = fmap2;
    a.B = B; a.D = D; a.H = H; a.W1 = W1; a.W2 = W2;
    a.nfused = nfused;
    if (f.rec) {
        a.rec = pyr[0];
        a.rec_nr = RC_REC_COUNT(W2);
    }
    const long rows = (long)B * H * W1;
    for (int l = 0; l < a.nfused && !f.rec; ++l) {
        a.lvl[l] = pyr[l];
        a.ld[l] = pyr_ld ? pyr_ld[l] : (W2 >> l);
        if ((f.shmask >> l & 1u) && pyr[l]) a.shadow[l] = shadow_offset(rows, a.ld[l], elem_size(f.kind));
        if (f.disp && pyr[l]) a.shk[l] = RC_SHEAR_ROWS(W2, W1, l);
    }
    a.tiles_m = (W1 + 127) / 128;
    a.tiles_n = (W2 + 127) / 128;
    set_sqrt_d(a, D);
    a.pyr_bf16 = f.kind;                        // the element kind
    hipStream_t s = hip_stream(stream);
    // fp32 fmaps + fp32 pyramid: exact fp32 MFMA.  bf16 fmaps, or a bf16
    // pyramid (bf16-level tolerance requested), take the bf16 MFMA kernel;
    // an fp16 pyramid (from fp16 or fp32 fmaps) its fp16 twin.
    const bool bf16_mma = fmap_dtype != RC_F32 || f.kind != RC_F32;
    // fp32: the split-bf16 kernel (fp32 accuracy, volume_split.hip) unless the
    // exact fp32 MFMA kernel is asked for or the shape is outside the split
    // kernel's addressing (hipErrorNotSupported: nothing was launched)
    hipError_t e = hipErrorNotSupported;
    if (bf16_mma) e = rc_launch_build_bf16mma(a, fmap_dtype != RC_F32, s);
    else if (!f.exact) e = rc_launch_build_split(a, s);
    if (e == hipErrorNotSupported && f.disp)
        return fail(RC_EUNSUPPORTED, "rc_corr_build: RC_LAYOUT_DISPARITY: shape outside the split build");
    if (e == hipErrorNotSupported && f.rec)
        return fail(RC_EUNSUPPORTED, "rc_corr_build: RC_LAYOUT_RECORDS: shape outside the records build");
    if (e == hipErrorNotSupported && !bf16_mma) e = rc_launch_build_f32(a, s);
    if (int rc = hip_rc(e, who, "volume launch")) return rc;
    for (int l = a.nfused; l < nbuf; ++l) {
        const long long ldi = pyr_ld ? pyr_ld[l - 1] : (W2 >> (l - 1));
        const long long ldo = pyr_ld ? pyr_ld[l] : (W2 >> l);
        // the level, then the same pooling step once more into its shadow copy
        const bool shadowed = (f.shmask >> l & 1u) && pyr[l];
        for (int copy = 0; copy <= (shadowed ? 1 : 0); ++copy) {
            void *out = copy ? static_cast<char *>(pyr[l]) + shadow_offset(rows, ldo, elem_size(a.pyr_bf16)) : pyr[l];
            if (int rc = hip_rc(rc_launch_pool(pyr[l - 1], ldi, out, ldo, rows, W2 >> (l - 1), a.pyr_bf16, s), who,
                                "pool launch"))
                return rc;
        }
    }
    return RC_OK;
}

extern "C" int rc_corr_pool(const void *in, long ld_in, void *out, long ld_out, long rows,
                            int W_in, int dtype, void *stream) {
    g_err[0] = 0;
    Flags f;
    if (int e = check_flags("rc_corr_pool", dtype, 0, f)) return e;   // pools the primary copy; a shadow is not written
    if (rows < 0 || W_in < 2 || ld_in < W_in || ld_out < W_in / 2)
        return fail(RC_EINVAL, "rc_corr_pool: bad shape rows=%ld W_in=%d ld_in=%ld ld_out=%ld", rows,
                    W_in, ld_in, ld_out);
    if (!known_kind(f.kind)) return fail(RC_EINVAL, "rc_corr_pool: unknown dtype %d", f.kind);
    if (rows == 0) return RC_OK;
    if (!in || !out) return fail(RC_EINVAL, "rc_corr_pool: null pointer");
    return hip_rc(rc_launch_pool(in, ld_in, out, ld_out, rows, W_in, f.kind, hip_stream(stream)), "rc_corr_pool",
                  "launch");
}

extern "C" int rc_corr_build_backward(const void *fmap1, const void *fmap2, int fmap_dtype, int B,
                                      int D, int H, int W1, int W2, const void *const *grad_pyr,
                                      const long *grad_ld, int levels, float *grad_fmap1,
                                      float *grad_fmap2, void *stream) {
    g_err[0] = 0;
    const unsigned shmask = shadow_mask(levels);   // RC_SHADOW_LEVEL bits (pair layout)
    levels &= 0xFF;
    if (B < 0 || D <= 0 || H < 0 || W1 < 0 || W2 <= 0)
        return fail(RC_EINVAL, "rc_corr_build_backward: bad shape B=%d D=%d H=%d W1=%d W2=%d", B, D,
                    H, W1, W2);
    const bool exact_f32 = (fmap_dtype & RC_BUILD_EXACT_F32) != 0;
    fmap_dtype &= ~RC_BUILD_EXACT_F32;
    if (fmap_dtype != RC_F32)
        return fail(RC_EUNSUPPORTED, "rc_corr_build_backward: fp32 feature maps only");
    if (levels < 1 || levels > RC_MAX_LEVELS || (W2 >> (levels - 1)) < 1)
        return fail(RC_EINVAL, "rc_corr_build_backward: levels=%d invalid for W2=%d", levels, W2);
    if (!grad_pyr) return fail(RC_EINVAL, "rc_corr_build_backward: null gradient array");
    if ((long long)B * H * W1 == 0) return RC_OK;   // nothing to reduce; outputs are empty
    if (!fmap1 || !fmap2 || !grad_fmap1 || !grad_fmap2 || !aligned16(fmap1) || !aligned16(fmap2) ||
        !aligned16(grad_fmap1) || !aligned16(grad_fmap2))
        return fail(RC_EINVAL, "rc_corr_build_backward: feature maps and their gradients must be "
                    "non-null and 16-byte aligned");
    rc::BuildBwdArgs a{};
    // levels == 3 with grad_pyr[1] NULL: pair-folded gradients (levels 0, 2)
    const bool pair = levels == 3 && !grad_pyr[1];
    if (shmask && (!pair || (shmask & ~0x5u)))
        return fail(RC_EUNSUPPORTED, "rc_corr_build_backward: RC_SHADOW copies are levels 0 and 2 of "
                    "the pair layout");
    for (int l = 0; l < levels; ++l) {
        const long ld = grad_ld ? grad_ld[l] : (long)(W2 >> l);
        if (pair && l == 1) {
            a.g[1] = nullptr;
            a.ld[1] = W2 >> 1;
            a.Wl[1] = W2 >> 1;
            continue;
        }
        if (!grad_pyr[l] || !aligned16(grad_pyr[l]))
            return fail(RC_EINVAL, "rc_corr_build_backward: level gradient %d null or not 16-byte "
                        "aligned", l);
        if (ld < (long)(W2 >> l))
            return fail(RC_EINVAL, "rc_corr_build_backward: row stride %ld of level %d < width %d",
                        ld, l, W2 >> l);
        a.g[l] = static_cast<const float *>(grad_pyr[l]);
        a.ld[l] = ld;
        a.Wl[l] = W2 >> l;
        if (shmask >> l & 1u) a.shadow[l] = shadow_offset((long long)B * H * W1, ld, 4) / 4;
    }
    if (a.ld[0] % 4 != 0)
        return fail(RC_EINVAL, "rc_corr_build_backward: level-0 row stride %lld is not a multiple "
                    "of 4", a.ld[0]);
    a.nlev = levels;
    a.exact = exact_f32 ? 1 : 0;
    a.f1 = static_cast<const float *>(fmap1);
    a.f2 = static_cast<const float *>(fmap2);
    a.df1 = grad_fmap1;
    a.df2 = grad_fmap2;
    a.B = B; a.D = D; a.H = H; a.W1 = W1; a.W2 = W2;
    a.tm = (D + 127) / 128;
    a.tn1 = (W1 + 127) / 128;
    a.tn2 = (W2 + 127) / 128;
    set_sqrt_d(a, D);
    return hip_rc(rc_launch_volume_bwd(a, hip_stream(stream)), "rc_corr_build_backward", "launch");
}

// ---- lookup --------------------------------------------------------------------------------------------------------
namespace {
// What prep_lookup lets pass on top of a full fp32 / bf16 pyramid: levels above
// 0 that are NULL (recomputed by the kernel, never read), an RC_F16 pyramid.
enum : unsigned { kNullLevels = 1, kF16Pyramid = 2 };

// Shared validation of the lookup entry points; fills `a` or returns an error.
// `io` is the tensor that must not be null (out / grad_out).
int prep_lookup(const char *who, const void *const *pyr, const int *widths, const long *pyr_ld,
                const Flags &f, unsigned allow, int levels, int radius, const float *coords_x,
                long coord_batch_stride, int B, int H, int W1, const void *io, rc::LookupArgs &a,
                bool *empty) {
    *empty = false;
    if (levels < 1 || levels > RC_MAX_LEVELS)
        return fail(RC_EINVAL, "%s: levels=%d outside 1..%d", who, levels, RC_MAX_LEVELS);
    if (radius < 1 || radius > 8)
        return fail(RC_EUNSUPPORTED, "%s: radius=%d outside 1..8", who, radius);
    if (!known_kind(f.kind)) return fail(RC_EINVAL, "%s: unknown pyramid dtype %d", who, f.kind);
    if (f.kind == RC_F16 && !(allow & kF16Pyramid))   // refused whatever the size, before any launch
        return fail(RC_EUNSUPPORTED, "%s: an RC_F16 pyramid is read by rc_corr_lookup and "
                    "rc_corr_lookup_chain only", who);
    if (B < 0 || H < 0 || W1 < 0)
        return fail(RC_EINVAL, "%s: bad shape B=%d H=%d W1=%d", who, B, H, W1);
    if (!pyr || !widths) return fail(RC_EINVAL, "%s: null pyramid/width array", who);
    const long long P = (long long)B * H * W1;
    if (P == 0) {
        *empty = true;
        return RC_OK;
    }
    if ((long long)H * W1 > 0x7FFFFFFF) return fail(RC_EUNSUPPORTED, "%s: H*W1 too large", who);
    if (!coords_x || !io) return fail(RC_EINVAL, "%s: null coords/out", who);
    a = rc::LookupArgs{};
    for (int i = 0; i < levels; ++i) {
        if (widths[i] < 1) return fail(RC_EINVAL, "%s: level %d width %d", who, i, widths[i]);
        if (!pyr[i] && (allow & kNullLevels) && i > 0) {
            a.lvl[i] = nullptr;
            a.W[i] = widths[i];
            a.ld[i] = widths[i];
            continue;
        }
        if (!pyr[i] || !aligned16(pyr[i]))
            return fail(RC_EINVAL, "%s: level %d null or not 16-byte aligned", who, i);
        a.lvl[i] = pyr[i];
        a.W[i] = widths[i];
        a.ld[i] = pyr_ld ? pyr_ld[i] : widths[i];
        if (f.rec) {
            if (i > 0) return fail(RC_EINVAL, "%s: RC_LAYOUT_RECORDS: pyr[%d] must be NULL", who, i);
            a.ld[0] = widths[0];
            a.rec_nr = RC_REC_COUNT(widths[0]);
            continue;
        }
        if (f.disp) {
            if (a.ld[i] < W1 || a.ld[i] % 4)
                return fail(RC_EINVAL, "%s: disparity-major row stride %lld of level %d must be >= W1 = %d "
                            "and a multiple of 4", who, a.ld[i], i, W1);
            a.shk[i] = RC_SHEAR_ROWS(widths[0], W1, i);
            if ((long long)B * H * a.shk[i] * a.ld[i] * 4 >= 0xFFFFFF00LL)
                return fail(RC_EUNSUPPORTED, "%s: disparity-major level %d exceeds 4 GiB", who, i);
            continue;
        }
        if (a.ld[i] < widths[i])
            return fail(RC_EINVAL, "%s: level %d row stride %lld < width %d", who, i, a.ld[i],
                        widths[i]);
        if (f.shmask >> i & 1u) {
            const int es = elem_size(f.kind);
            a.shadow[i] = shadow_offset(P, a.ld[i], es);
            // the pair kernel addresses both copies with 32-bit buffer offsets
            if (a.shadow[i] + P * a.ld[i] * es > 0xFFFFFF00LL)
                return fail(RC_EUNSUPPORTED, "%s: level %d with its shadow copy exceeds 4 GiB", who, i);
        }
    }
    a.coords = coords_x;
    a.cbs = coord_batch_stride;
    a.P = P;
    a.HW = H * W1;
    a.W1 = W1;
    a.levels = levels;
    return RC_OK;
}

// Which pool-chain kernel serves a request (rc_corr_lookup_chain and the
// chain mode of rc_corr_lookup_step): the pair kernel (reads levels 0 and 2)
// for 2 levels, or for 4 levels when level 2 is given; otherwise the level-1
// chain kernel (reads levels 0 and 1) for 3-4 levels.
int chain_kind(const char *who, const void *const *pyr, const int *widths, int levels, int radius,
               bool *pair, bool rec = false) {
    if (levels < 2 || levels > 4 || radius < 1 || radius > 4)
        return fail(RC_EUNSUPPORTED, "%s: levels 2..4 and radius 1..4 only", who);
    for (int i = 1; i < levels; ++i)
        if (widths[i] != widths[i - 1] / 2)
            return fail(RC_EINVAL, "%s: width %d of level %d is not floor(%d/2)", who, widths[i], i,
                        widths[i - 1]);
    *pair = levels == 2 || (levels == 4 && (pyr[2] != nullptr || rec));
    // the pair kernel's window argument holds for widths up to 2^16 (lookup.hip)
    if (*pair && widths[0] > 65536)
        return fail(RC_EUNSUPPORTED, "%s: level-0 width %d > 65536 for the pair kernel", who,
                    widths[0]);
    if (!*pair && !pyr[1])
        return fail(RC_EINVAL, "%s: %d levels need level 1 (or level 2 with 4 levels)", who, levels);
    if (!*pair && levels < 3)
        return fail(RC_EUNSUPPORTED, "%s: the level-1 chain needs 3..4 levels", who);
    return RC_OK;
}

// Row strides the chain kernels read with 16-B chunks must be whole chunks
// (multiples of 4 fp32 / 8 bf16 or fp16 elements).
int chain_strides(const char *who, const rc::LookupArgs &a, bool pair, bool bf16 = false) {
    const int need[2] = {0, pair ? 2 : 1};
    const int epc = bf16 ? 8 : 4;
    for (int k = 0; k < 2; ++k) {
        const int i = need[k];
        if (i < a.levels && a.ld[i] % epc != 0)
            return fail(RC_EINVAL, "%s: level-%d row stride %lld is not a multiple of %d", who, i,
                        a.ld[i], epc);
    }
    return RC_OK;
}
}  // namespace

extern "C" int rc_corr_lookup(const void *const *pyr, const int *widths, const long *pyr_ld,
                              int pyr_dtype, int levels, int radius, const float *coords_x,
                              long coord_batch_stride, int B, int H, int W1, float *out,
                              void *stream) {
    g_err[0] = 0;
    const char *who = "rc_corr_lookup";
    Flags f;
    rc::LookupArgs a;
    bool empty;
    if (int e = check_flags(who, pyr_dtype, 0, f)) return e;
    int rc = prep_lookup(who, pyr, widths, pyr_ld, f, kF16Pyramid, levels, radius, coords_x, coord_batch_stride,
                         B, H, W1, out, a, &empty);
    if (rc || empty) return rc;
    a.out = out;
    hipStream_t s = hip_stream(stream);
    return hip_rc(f.kind == RC_F16 ? rc_launch_lookup_f16pyr(a, radius, s)
                                   : rc_launch_lookup(a, radius, f.kind == RC_BF16, s),
                  who, "launch");
}

extern "C" int rc_corr_lookup_chain(const void *const *pyr, const int *widths, const long *pyr_ld,
                                    int pyr_dtype, int levels, int radius, const float *coords_x,
                                    long coord_batch_stride, int B, int H, int W1, void *out,
                                    void *stream) {
    g_err[0] = 0;
    const char *who = "rc_corr_lookup_chain";
    Flags f;
    rc::LookupArgs a;
    bool empty;
    if (int e = check_flags(who, pyr_dtype, RC_OUT_CHANNELS_LAST | RC_OUT_F16 | RC_OUT_BF16 | RC_LAYOUT_DISPARITY |
                                                RC_LAYOUT_RECORDS, f))
        return e;
    int rc = prep_lookup(who, pyr, widths, pyr_ld, f, kNullLevels | kF16Pyramid, levels, radius, coords_x,
                         coord_batch_stride, B, H, W1, out, a, &empty);
    if (rc) return rc;
    bool pair;
    if ((rc = chain_kind(who, pyr, widths, levels, radius, &pair, f.rec))) return rc;
    if (f.rec && (levels != 4 || f.kind != RC_BF16 || f.shmask))
        return fail(RC_EUNSUPPORTED, "rc_corr_lookup_chain: RC_LAYOUT_RECORDS needs the 4-level bf16 pair "
                    "layout and no shadow copies");
    if (f.disp && (!pair || f.kind != RC_F32 || f.cl || f.shmask))
        return fail(RC_EUNSUPPORTED, "rc_corr_lookup_chain: RC_LAYOUT_DISPARITY needs the fp32 pair layout "
                    "(2 levels, or 4 with level 2 given), NCHW output and no shadow copies");
    if (f.kind != RC_F32 && !pair)
        return fail(RC_EUNSUPPORTED, "rc_corr_lookup_chain: a bf16 / fp16 pyramid needs the pair layout "
                    "(2 levels, or 4 with level 2 given)");
    if (f.cl && !pair)
        return fail(RC_EUNSUPPORTED, "rc_corr_lookup_chain: RC_OUT_CHANNELS_LAST needs the pair layout");
    if (f.out_dt && (!pair || f.disp))
        return fail(RC_EUNSUPPORTED, "rc_corr_lookup_chain: RC_OUT_F16 / RC_OUT_BF16 need the pair layout "
                    "(2 levels, or 4 with level 2 given) in rows or records");
    if (empty) return RC_OK;
    a.out = static_cast<float *>(out);
    a.out_cl = f.cl;
    a.out_dt = f.out_dt;
    if (!f.rec && (rc = chain_strides(who, a, pair, f.kind != RC_F32))) return rc;
    hipStream_t s = hip_stream(stream);
    return hip_rc(pair ? (f.kind == RC_F16 ? rc_launch_lookup_pair_f16pyr(a, radius, s)
                                           : rc_launch_lookup_pair(a, radius, f.kind == RC_BF16, s))
                       : rc_launch_lookup_chain(a, radius, s),
                  who, "launch");
}

extern "C" int rc_corr_lookup_step(const void *const *pyr, const int *widths, const long *pyr_ld,
                                   int pyr_dtype, int levels, int radius, int chain,
                                   const float *coords1, const float *delta, float *coords1_out,
                                   float *flow_out, int B, int H, int W1, void *out,
                                   void *stream) {
    g_err[0] = 0;
    const char *who = "rc_corr_lookup_step";
    Flags f;
    rc::LookupArgs a;
    bool empty;
    if (int e = check_flags(who, pyr_dtype, RC_OUT_CHANNELS_LAST | RC_OUT_F16 | RC_OUT_BF16 | RC_LAYOUT_RECORDS, f))
        return e;
    if (f.rec && !chain) return fail(RC_EUNSUPPORTED, "rc_corr_lookup_step: RC_LAYOUT_RECORDS needs chain != 0");
    if (f.out_dt && !chain)
        return fail(RC_EUNSUPPORTED, "rc_corr_lookup_step: RC_OUT_F16 / RC_OUT_BF16 need chain != 0");
    int rc = prep_lookup(who, pyr, widths, pyr_ld, f, chain ? kNullLevels : 0u, levels, radius, coords1,
                         2L * H * W1, B, H, W1, out, a, &empty);
    if (rc) return rc;
    // the kernel that serves a chain call, asked once: before the size is looked
    // at when it decides a refusal (below), else after
    bool pair = false;
    auto kind = [&] { return chain ? chain_kind(who, pyr, widths, levels, radius, &pair, f.rec) : RC_OK; };
    if (f.out_dt) {   // out-dtype refusals come before the empty return, whatever the size
        if ((rc = kind())) return rc;
        if (!pair)
            return fail(RC_EUNSUPPORTED, "rc_corr_lookup_step: RC_OUT_F16 / RC_OUT_BF16 need the pair layout "
                        "(2 levels, or 4 with level 2 given) in rows or records");
    }
    if (empty) return RC_OK;
    if (!coords1_out || !flow_out)
        return fail(RC_EINVAL, "rc_corr_lookup_step: null coords1_out / flow_out");
    if (!f.out_dt && (rc = kind())) return rc;
    if (chain) {
        if (f.kind != RC_F32 && !pair)
            return fail(RC_EUNSUPPORTED, "rc_corr_lookup_step: a bf16 pyramid needs the pair layout");
        if (f.rec && (levels != 4 || f.kind != RC_BF16 || f.shmask))
            return fail(RC_EUNSUPPORTED, "rc_corr_lookup_step: RC_LAYOUT_RECORDS needs the 4-level bf16 pair "
                        "layout and no shadow copies");
        if (!f.rec && (rc = chain_strides(who, a, pair, f.kind == RC_BF16))) return rc;
    }
    if (f.cl && !pair)
        return fail(RC_EUNSUPPORTED, "rc_corr_lookup_step: RC_OUT_CHANNELS_LAST needs the pair layout");
    a.out = static_cast<float *>(out);
    a.out_cl = f.cl;
    a.out_dt = f.out_dt;
    a.step = 1;
    a.W1 = W1;
    a.delta = delta;
    a.coords_out = coords1_out;
    a.flow_out = flow_out;
    hipStream_t s = hip_stream(stream);
    return hip_rc(chain ? (pair ? rc_launch_lookup_pair(a, radius, f.kind == RC_BF16, s)
                                : rc_launch_lookup_chain(a, radius, s))
                        : rc_launch_lookup(a, radius, f.kind == RC_BF16, s),
                  who, "launch");
}

// ---- lookup backward -----------------------------------------------------------------------------------------------
namespace {
// Validation shared by rc_corr_lookup_backward and rc_corr_lookup_backward_calls.
int prep_lookup_bwd(const char *who, void *const *grad_pyr, const int *widths, const long *grad_ld,
                    int levels, int radius, const float *coords_x, long coord_batch_stride, int B,
                    int H, int W1, const float *grad_out, rc::LookupBwdArgs &a, bool *empty,
                    bool *pair_out) {
    // RC_SHADOW_LEVEL(l) bits above the level count: gradient copies (pair layout)
    const unsigned shmask = shadow_mask(levels);
    levels &= 0xFF;
    rc::LookupArgs la;
    int rc = prep_lookup(who, grad_pyr, widths, grad_ld, decode_flags(RC_F32), kNullLevels, levels, radius,
                         coords_x, coord_batch_stride, B, H, W1, grad_out, la, empty);
    if (rc || *empty) return rc;
    // pair-folded buffers: levels 1 and 3 NULL, their gradients folded into
    // levels 0 and 2 (2 or 4 levels, radius 1..4, widths halving, W <= 2^16)
    const bool pair = levels >= 2 && !grad_pyr[1];
    *pair_out = pair;
    if (pair) {
        bool ok = (levels == 2 || (levels == 4 && grad_pyr[2] && !grad_pyr[3])) && radius <= 4 &&
                  widths[0] <= 65536;
        for (int i = 1; i < levels; ++i) ok = ok && widths[i] == widths[i - 1] / 2;
        if (!ok)
            return fail(RC_EINVAL, "%s: NULL gradient levels need the pair layout (levels 2 or 4, "
                        "level 1 [and 3] NULL, radius <= 4, halving widths)", who);
        if (shmask && (levels != 4 || (shmask & ~0x5u)))
            return fail(RC_EUNSUPPORTED, "%s: RC_SHADOW gradient copies are levels 0 and 2 of the "
                        "4-level pair layout", who);
    } else if (shmask) {
        return fail(RC_EUNSUPPORTED, "%s: RC_SHADOW needs the pair layout", who);
    } else {
        for (int i = 1; i < levels; ++i)
            if (!grad_pyr[i]) return fail(RC_EINVAL, "%s: level %d null", who, i);
    }
    a = rc::LookupBwdArgs{};
    for (int i = 0; i < levels; ++i) {
        a.W[i] = la.W[i];
        a.ld[i] = la.ld[i];
        if (!grad_pyr[i]) {
            a.g[i] = nullptr;
            continue;
        }
        if (la.ld[i] % 4 != 0)
            return fail(RC_EINVAL, "%s: row stride %lld of level %d is not a multiple of 4", who,
                        la.ld[i], i);
        a.g[i] = static_cast<float *>(const_cast<void *>(la.lvl[i]));
        if (shmask >> i & 1u) {
            a.shadow[i] = shadow_offset(la.P, la.ld[i], 4);
            if (a.shadow[i] + la.P * la.ld[i] * 4 > 0xFFFFFF00LL)
                return fail(RC_EUNSUPPORTED, "%s: level %d with its shadow copy exceeds 4 GiB", who, i);
        }
    }
    a.coords = coords_x;
    a.cbs = coord_batch_stride;
    a.grad_out = grad_out;
    a.P = la.P;
    a.HW = la.HW;
    a.levels = levels;
    return RC_OK;
}
}  // namespace

extern "C" int rc_corr_lookup_backward(void *const *grad_pyr, const int *widths,
                                       const long *grad_ld, int levels, int radius,
                                       const float *coords_x, long coord_batch_stride, int B,
                                       int H, int W1, const float *grad_out, void *stream) {
    g_err[0] = 0;
    if (levels & ~0xFFFF)
        return fail(RC_EINVAL, "rc_corr_lookup_backward: unknown flag bits 0x%x", levels & ~0xFFFF);
    rc::LookupBwdArgs a;
    bool empty = false, pair = false;
    int rc = prep_lookup_bwd("rc_corr_lookup_backward", grad_pyr, widths, grad_ld, levels, radius,
                             coords_x, coord_batch_stride, B, H, W1, grad_out, a, &empty, &pair);
    if (rc || empty) return rc;
    return hip_rc(rc_launch_lookup_bwd(a, radius, hip_stream(stream)), "rc_corr_lookup_backward", "launch");
}

extern "C" int rc_corr_lookup_backward_calls(void *const *grad_pyr, const int *widths,
                                             const long *grad_ld, int levels, int radius,
                                             int n_calls, const float *const *coords_x,
                                             const long *coord_batch_stride, int B, int H, int W1,
                                             const float *const *grad_out, void *stream) {
    g_err[0] = 0;
    const char *who = "rc_corr_lookup_backward_calls";
    const bool overwrite = (levels & RC_GRAD_OVERWRITE) != 0;
    levels &= ~RC_GRAD_OVERWRITE;
    if (levels & ~0xFFFF) return fail(RC_EINVAL, "%s: unknown flag bits 0x%x", who, levels & ~0xFFFF);
    if (n_calls < 0) return fail(RC_EINVAL, "%s: n_calls=%d", who, n_calls);
    if (n_calls > 0 && (!coords_x || !coord_batch_stride || !grad_out))
        return fail(RC_EINVAL, "%s: null coords / stride / grad_out array", who);
    if (levels & 0xFF00) return fail(RC_EUNSUPPORTED, "%s: RC_SHADOW gradient copies", who);
    const hipStream_t s = hip_stream(stream);
    rc::LookupBwdArgs a;
    bool empty = false, pair = false;
    for (int c = 0; c < n_calls; ++c) {       // every call validated before any launch
        int rc = prep_lookup_bwd(who, grad_pyr, widths, grad_ld, levels, radius, coords_x[c],
                                 coord_batch_stride[c], B, H, W1, grad_out[c], a, &empty, &pair);
        if (rc || empty) return rc;
    }
    if (n_calls == 0) {
        if (overwrite) return fail(RC_EINVAL, "%s: RC_GRAD_OVERWRITE with no calls", who);
        return RC_OK;
    }
    auto per_call = [&]() -> int {
        // per-level layout, or rows too wide for LDS: zero if asked, then one
        // rc_corr_lookup_backward launch per call
        if (overwrite)
            for (int i = 0; i < a.levels; ++i)
                if (a.g[i])
                    if (int rc = hip_rc(hipMemsetAsync(a.g[i], 0, (size_t)(a.P * a.ld[i]) * 4, s), who, "memset"))
                        return rc;
        for (int c = 0; c < n_calls; ++c) {
            a.coords = coords_x[c];
            a.cbs = coord_batch_stride[c];
            a.grad_out = grad_out[c];
            if (int rc = hip_rc(rc_launch_lookup_bwd(a, radius, s), who, "launch")) return rc;
        }
        return RC_OK;
    };
    if (!pair) return per_call();
    rc::LookupBwdCallsArgs ca{};
    ca.g[0] = a.g[0];
    ca.ld[0] = a.ld[0];
    if (a.levels == 4) {
        ca.g[1] = a.g[2];
        ca.ld[1] = a.ld[2];
    }
    for (int i = 0; i < a.levels; ++i) ca.W[i] = a.W[i];
    ca.P = a.P;
    ca.HW = a.HW;
    // fused or per-call for the WHOLE request, decided before any launch
    if (!rc_lookup_bwd_calls_fits(ca, radius, a.levels, coord_batch_stride, n_calls)) return per_call();
    for (int c0 = 0; c0 < n_calls; c0 += rc::kMaxBwdCalls) {
        ca.ncalls = std::min(rc::kMaxBwdCalls, n_calls - c0);
        ca.accumulate = (c0 > 0 || !overwrite) ? 1 : 0;
        for (int c = 0; c < ca.ncalls; ++c) {
            ca.coords[c] = coords_x[c0 + c];
            ca.cbs[c] = coord_batch_stride[c0 + c];
            ca.grad_out[c] = grad_out[c0 + c];
        }
        if (int rc = hip_rc(rc_launch_lookup_bwd_calls(ca, radius, a.levels, s), who, "launch")) return rc;
    }
    return RC_OK;
}

// ---- conv: the lookup fused with convc1, and its backward ------------------------------------------------------------
namespace {
// Shared validation of rc_corr_lookup_chain_conv and its backward: the pair
// layout in rows (2 levels, or 4 with level 2 given), rc_corr_lookup_chain's
// checks.  Every refusal comes before the empty-problem return, so it does
// not depend on B.  `io` is the tensor that must not be null (out / grad_out).
int prep_chain_conv(const char *who, const void *const *pyr, const int *widths, const long *pyr_ld,
                    int pyr_dtype, int levels, int radius, const float *coords_x, long coord_batch_stride,
                    int B, int H, int W1, const void *io, bool allow_half, Flags &f, rc::LookupArgs &a,
                    bool *empty) {
    f = decode_flags(pyr_dtype);
    if (f.cl) return fail(RC_EUNSUPPORTED, "%s: RC_OUT_CHANNELS_LAST: the fused output is NCHW only", who);
    if (f.rec || f.disp)
        return fail(RC_EUNSUPPORTED, "%s: RC_LAYOUT_RECORDS / RC_LAYOUT_DISPARITY: the fused lookup reads "
                    "the pair layout in rows only", who);
    if (!allow_half && f.out_dt)
        return fail(RC_EUNSUPPORTED, "%s: RC_OUT_F16 / RC_OUT_BF16: grad_out and the gradients are fp32", who);
    // what is left: the two RC_OUT_* flags at once, and bits no entry point knows
    if (int e = check_flags(who, pyr_dtype, RC_OUT_HALF, f)) return e;
    int rc = prep_lookup(who, pyr, widths, pyr_ld, f, kNullLevels, levels, radius, coords_x, coord_batch_stride,
                         B, H, W1, io, a, empty);
    if (rc) return rc;
    if (levels == 3)
        return fail(RC_EUNSUPPORTED, "%s: 3 levels are the level-1 chain; the fused pair kernels serve 2 "
                    "levels, or 4 with level 2 given (rc_corr_lookup_conv reads a full pyramid)", who);
    if (levels == 4 && !pyr[2])
        return fail(RC_EUNSUPPORTED, "%s: 4 levels need level 2 (the pair layout); rc_corr_lookup_conv "
                    "reads a full pyramid", who);
    bool pair = false;
    if ((rc = chain_kind(who, pyr, widths, levels, radius, &pair))) return rc;
    if (!pair) return fail(RC_EUNSUPPORTED, "%s: the pair layout only (2 levels, or 4 with level 2 given)", who);
    return RC_OK;
}

// What the two conv backward entry points check after their lookup arguments:
// cout, that something is asked for, then either the empty problem (the sums
// over no pixels are zeros: memsets on the caller's stream, RC_OK) or the
// weight and the workspace of a real one.
int conv_bwd_request(const char *who, int levels, int radius, int cout, bool empty, const float *weight,
                     const float *grad_corr, float *grad_weight, float *grad_bias, const float *workspace,
                     hipStream_t s) {
    if (cout < 1 || cout > (1 << 20)) return fail(RC_EINVAL, "%s: cout=%d", who, cout);
    if (!grad_corr && !grad_weight && !grad_bias)
        return fail(RC_EINVAL, "%s: none of grad_corr, grad_weight, grad_bias requested", who);
    if (empty) {
        const size_t cin = (size_t)levels * (2 * radius + 1);
        if (grad_weight)
            if (int rc = hip_rc(hipMemsetAsync(grad_weight, 0, (size_t)cout * cin * sizeof(float), s), who, "memset"))
                return rc;
        if (grad_bias)
            if (int rc = hip_rc(hipMemsetAsync(grad_bias, 0, (size_t)cout * sizeof(float), s), who, "memset"))
                return rc;
        return RC_OK;
    }
    if (!weight) return fail(RC_EINVAL, "%s: null weight", who);
    if ((grad_weight || grad_bias) && !workspace)
        return fail(RC_EINVAL, "%s: grad_weight / grad_bias need a workspace of "
                    "RC_LOOKUP_CONV_BWD_WS(P, cout, cin) floats", who);
    return RC_OK;
}
}  // namespace

extern "C" int rc_corr_lookup_conv(const void *const *pyr, const int *widths, const long *pyr_ld,
                                   int pyr_dtype, int levels, int radius, const float *coords_x,
                                   long coord_batch_stride, int B, int H, int W1,
                                   const float *weight, const float *bias, int cout, int relu,
                                   float *out, void *stream) {
    g_err[0] = 0;
    const char *who = "rc_corr_lookup_conv";
    Flags f;
    rc::LookupArgs a;
    bool empty;
    if (int e = check_flags(who, pyr_dtype, 0, f)) return e;
    int rc = prep_lookup(who, pyr, widths, pyr_ld, f, 0u, levels, radius, coords_x, coord_batch_stride, B, H, W1,
                         out, a, &empty);
    if (rc) return rc;
    if (levels < 2 || levels > 4 || radius > 4)
        return fail(RC_EUNSUPPORTED, "rc_corr_lookup_conv: levels 2..4 and radius 1..4 only");
    if (cout < 1) return fail(RC_EINVAL, "rc_corr_lookup_conv: cout=%d", cout);
    if (empty) return RC_OK;
    if (!weight) return fail(RC_EINVAL, "rc_corr_lookup_conv: null weight");
    return hip_rc(rc_launch_lookup_conv(a, radius, f.kind == RC_BF16, weight, bias, cout, relu, out,
                                        hip_stream(stream)),
                  who, "launch");
}

extern "C" int rc_corr_lookup_conv_backward(const void *const *pyr, const int *widths, const long *pyr_ld,
                                            int pyr_dtype, int levels, int radius, const float *coords_x,
                                            long coord_batch_stride, int B, int H, int W1,
                                            const float *weight, const float *bias, int cout, int relu,
                                            const float *grad_out, float *grad_corr, float *grad_weight,
                                            float *grad_bias, float *workspace, void *stream) {
    g_err[0] = 0;
    const char *who = "rc_corr_lookup_conv_backward";
    Flags f;
    rc::LookupArgs a;
    bool empty;
    if (int e = check_flags(who, pyr_dtype, 0, f)) return e;
    int rc = prep_lookup(who, pyr, widths, pyr_ld, f, 0u, levels, radius, coords_x, coord_batch_stride, B, H, W1,
                         grad_out, a, &empty);
    if (rc) return rc;
    if (levels < 2 || levels > 4 || radius > 4)
        return fail(RC_EUNSUPPORTED, "%s: levels 2..4 and radius 1..4 only", who);
    hipStream_t s = hip_stream(stream);
    rc = conv_bwd_request(who, levels, radius, cout, empty, weight, grad_corr, grad_weight, grad_bias, workspace, s);
    if (rc || empty) return rc;
    return hip_rc(rc_launch_lookup_conv_bwd(a, radius, f.kind == RC_BF16, weight, bias, cout, relu,
                                            grad_out, grad_corr, grad_weight, grad_bias, workspace, s),
                  who, "launch");
}

extern "C" int rc_corr_lookup_chain_conv(const void *const *pyr, const int *widths, const long *pyr_ld,
                                         int pyr_dtype, int levels, int radius, const float *coords_x,
                                         long coord_batch_stride, int B, int H, int W1,
                                         const float *weight, const float *bias, int cout, int relu,
                                         void *out, void *stream) {
    g_err[0] = 0;
    const char *who = "rc_corr_lookup_chain_conv";
    Flags f;
    rc::LookupArgs a;
    bool empty;
    int rc = prep_chain_conv(who, pyr, widths, pyr_ld, pyr_dtype, levels, radius, coords_x,
                             coord_batch_stride, B, H, W1, out, true, f, a, &empty);
    if (rc) return rc;
    if (cout < 1) return fail(RC_EINVAL, "%s: cout=%d", who, cout);
    if (empty) return RC_OK;
    if (!weight) return fail(RC_EINVAL, "%s: null weight", who);
    if ((rc = chain_strides(who, a, true, f.kind == RC_BF16))) return rc;
    a.out = static_cast<float *>(out);
    a.out_dt = f.out_dt;
    return hip_rc(rc_launch_lookup_pair_conv(a, radius, f.kind == RC_BF16, weight, bias, cout, relu,
                                             hip_stream(stream)),
                  who, "launch");
}

extern "C" int rc_corr_lookup_chain_conv_backward(const void *const *pyr, const int *widths,
                                                  const long *pyr_ld, int pyr_dtype, int levels, int radius,
                                                  const float *coords_x, long coord_batch_stride, int B,
                                                  int H, int W1, const float *weight, const float *bias,
                                                  int cout, int relu, const float *grad_out,
                                                  float *grad_corr, float *grad_weight, float *grad_bias,
                                                  float *workspace, void *stream) {
    g_err[0] = 0;
    const char *who = "rc_corr_lookup_chain_conv_backward";
    Flags f;
    rc::LookupArgs a;
    bool empty;
    int rc = prep_chain_conv(who, pyr, widths, pyr_ld, pyr_dtype, levels, radius, coords_x,
                             coord_batch_stride, B, H, W1, grad_out, false, f, a, &empty);
    if (rc) return rc;
    hipStream_t s = hip_stream(stream);
    rc = conv_bwd_request(who, levels, radius, cout, empty, weight, grad_corr, grad_weight, grad_bias, workspace, s);
    if (rc || empty) return rc;
    if ((rc = chain_strides(who, a, true, f.kind == RC_BF16))) return rc;
    return hip_rc(rc_launch_lookup_pair_conv_bwd(a, radius, f.kind == RC_BF16, weight, bias, cout, relu, grad_out,
                                                 grad_corr, grad_weight, grad_bias, workspace, s),
                  who, "launch");
}

// ---- upsample ------------------------------------------------------------------------------------------------------
namespace {
// The checks of the two upsample entry points: shape and factor; the backward's
// complaint about what it is asked for (`request`, null when there is none);
// then *empty (RC_OK, nothing to do), or flow, mask and `io` (out / grad_out) must
// be there, `io` aligned: the kernels store / load the f values of a sub-row as one vector.
int prep_upsample(const char *who, const float *flow, const float *mask, const float *io, const char *io_name,
                  int N, int C, int H, int W, int factor, const char *request, bool *empty) {
    *empty = false;
    if (N < 0 || C < 1 || H < 0 || W < 0)
        return fail(RC_EINVAL, "%s: bad shape N=%d C=%d H=%d W=%d", who, N, C, H, W);
    if (factor != 1 && factor != 2 && factor != 4 && factor != 8)
        return fail(RC_EUNSUPPORTED, "%s: factor %d (1, 2, 4 or 8)", who, factor);
    if (request) return fail(RC_EINVAL, "%s: %s", who, request);
    *empty = (long long)N * H * W == 0;
    if (*empty) return RC_OK;
    if (!flow || !mask || !io) return fail(RC_EINVAL, "%s: null pointer", who);
    const int align = 4 * std::min(factor, 4);
    if (reinterpret_cast<uintptr_t>(io) & (uintptr_t)(align - 1))
        return fail(RC_EINVAL, "%s: %s must be %d-byte aligned", who, io_name, align);
    return RC_OK;
}
}  // namespace

extern "C" int rc_convex_upsample(const float *flow, const float *mask, int N, int C, int H, int W,
                                  int factor, float *out, void *stream) {
    g_err[0] = 0;
    const char *who = "rc_convex_upsample";
    bool empty;
    int rc = prep_upsample(who, flow, mask, out, "out", N, C, H, W, factor, nullptr, &empty);
    if (rc || empty) return rc;
    return hip_rc(rc_launch_convex_upsample(flow, mask, N, C, H, W, factor, out, hip_stream(stream)), who, "launch");
}

extern "C" int rc_convex_upsample_backward(const float *flow, const float *mask, const float *grad_out,
                                           int N, int C, int H, int W, int factor, float *grad_flow,
                                           float *grad_mask, float *workspace, void *stream) {
    g_err[0] = 0;
    const char *who = "rc_convex_upsample_backward";
    const char *request = nullptr;
    if (!grad_flow && !grad_mask) request = "neither grad_flow nor grad_mask requested";
    else if (grad_flow && !workspace) request = "grad_flow needs a workspace of RC_UPSAMPLE_BWD_WS(N, C, H, W) floats";
    bool empty;
    int rc = prep_upsample(who, flow, mask, grad_out, "grad_out", N, C, H, W, factor, request, &empty);
    if (rc || empty) return rc;
    return hip_rc(rc_launch_convex_upsample_bwd(flow, mask, grad_out, N, C, H, W, factor, grad_flow,
                                                grad_mask, workspace, hip_stream(stream)),
                  who, "launch");
}

extern "C" int rc_upsample_head(const float *flow, const long *flow_strides, const void *mask,
                                const long *mask_strides, int mask_dtype, float scale, int N, int C, int H,
                                int W, int factor, float *out, void *stream) {
    g_err[0] = 0;
    const char *who = "rc_upsample_head";
    if (!known_kind(mask_dtype))
        return fail(RC_EINVAL, "%s: unknown mask dtype %d (RC_F32, RC_F16 or RC_BF16)", who, mask_dtype);
    if (N < 0 || C < 1 || H < 0 || W < 0)
        return fail(RC_EINVAL, "%s: bad shape N=%d C=%d H=%d W=%d", who, N, C, H, W);
    if (factor != 1 && factor != 2 && factor != 4 && factor != 8)
        return fail(RC_EINVAL, "%s: factor %d (1, 2, 4 or 8)", who, factor);
    if (!flow_strides || !mask_strides) return fail(RC_EINVAL, "%s: null stride array", who);
    if (flow_strides[0] < 0 || flow_strides[1] < 0 || mask_strides[0] < 0 || mask_strides[1] < 0 ||
        mask_strides[2] < 0)
        return fail(RC_EINVAL, "%s: negative stride", who);
    // the mask's layout class; a stride along an axis of length 1 is ignored
    const long long HW = (long long)H * W, MC = 9LL * factor * factor;
    const bool planar = (HW <= 1 || mask_strides[2] == 1) && (HW == 0 || mask_strides[1] == HW);
    const bool inter = mask_strides[1] == 1 && (HW <= 1 || mask_strides[2] == MC);
    if (!planar && !inter)
        return fail(RC_EUNSUPPORTED, "%s: mask strides (%ld, %ld, %ld) are of neither layout class: planar "
                    "(channel stride H*W, pixel stride 1) or interleaved (channel stride 1, pixel stride 9 f^2)",
                    who, mask_strides[0], mask_strides[1], mask_strides[2]);
    if ((long long)N * HW == 0) return RC_OK;
    if (!flow || !mask || !out) return fail(RC_EINVAL, "%s: null pointer", who);
    if (!elem_aligned(flow, RC_F32) || !elem_aligned(mask, mask_dtype))
        return fail(RC_EINVAL, "%s: flow or mask is not aligned to its element size", who);
    const int align = 4 * std::min(factor, 4);
    if (reinterpret_cast<uintptr_t>(out) & (uintptr_t)(align - 1))
        return fail(RC_EINVAL, "%s: out must be %d-byte aligned", who, align);
    if ((long long)N * HW > (1LL << 36))
        return fail(RC_EUNSUPPORTED, "%s: N*H*W = %lld pixels exceed 2^36", who, (long long)N * HW);
    rc::HeadArgs a{flow, flow_strides[0], flow_strides[1], mask, mask_strides[0], scale, out, N, C, H, W, 0};
    return hip_rc(rc_launch_upsample_head(a, mask_dtype, factor, !planar, hip_stream(stream)), who, "launch");
}

// ---- gru: the gates, the blend, the input assembly, and their backward ---------------------------------------------
namespace {
// The checks of rc_gru_gates / rc_gru_blend and their backward entry points on
// their nops operands; fills `a` (rc::GruArgs or rc::GruBwdArgs).  *empty:
// nothing to do (RC_OK).
template <class Args>
int prep_gru(const char *who, void *const *ops, const char *const *names, int nops, const long *strides,
             int dtype, int N, int C, long HW, Args &a, bool *empty) {
    if (!known_kind(dtype))
        return fail(RC_EINVAL, "%s: unknown dtype %d (RC_F32, RC_F16 or RC_BF16)", who, dtype);
    if (N < 0 || C < 1 || HW < 0) return fail(RC_EINVAL, "%s: bad shape N=%d C=%d HW=%ld", who, N, C, HW);
    if (!strides) return fail(RC_EINVAL, "%s: null stride array", who);
    bool planar = true, inter = true;
    for (int k = 0; k < nops; ++k) {
        const long *t = strides + 3 * k;
        if (t[0] < 0 || t[1] < 0 || t[2] < 0)
            return fail(RC_EINVAL, "%s: negative stride of %s (%ld, %ld, %ld)", who, names[k], t[0], t[1], t[2]);
        planar = planar && (HW <= 1 || t[2] == 1);
        inter = inter && (C == 1 || t[1] == 1);
    }
    if (!planar && !inter)
        return fail(RC_EUNSUPPORTED, "%s: the operands share no layout class: every pixel stride 1 (planar) "
                    "or every channel stride 1 (interleaved)", who);
    *empty = (long long)N * HW == 0;
    if (*empty) return RC_OK;
    if (HW > 0x7FFFFFFFL || (long long)N * C * HW > 0xFFFFFFFFLL)
        return fail(RC_EUNSUPPORTED, "%s: N*C*HW = %lld elements exceed 2^32 - 1", who, (long long)N * C * HW);
    a.N = N;
    a.O = (uint32_t)(planar ? C : HW);
    a.L = planar ? HW : C;
    for (int k = 0; k < nops; ++k) {
        if (!ops[k]) return fail(RC_EINVAL, "%s: null %s", who, names[k]);
        if (!elem_aligned(ops[k], dtype))
            return fail(RC_EINVAL, "%s: %s is not aligned to its element size", who, names[k]);
        a.op[k] = rc::GruOperand{ops[k], strides[3 * k], strides[3 * k + (planar ? 1 : 2)]};
    }
    return RC_OK;
}

// an input among the operands: GruOperand holds inputs and outputs alike
void *mut(const void *p) { return const_cast<void *>(p); }

// rc_gru_gates (7 operands) and rc_gru_blend (5): prep_gru, then the launch.
int gru_forward(const char *who, void *const *ops, const char *const *names, int nops, const long *strides,
                int dtype, int N, int C, long HW, bool blend, void *stream) {
    g_err[0] = 0;
    rc::GruArgs a;
    bool empty;
    if (int rc = prep_gru(who, ops, names, nops, strides, dtype, N, C, HW, a, &empty)) return rc;
    if (empty) return RC_OK;
    if (!blend && ops[6] == ops[4]) return fail(RC_EINVAL, "%s: rh_out must not alias h (the blend reads h)", who);
    return hip_rc(rc_launch_gru(a, dtype, blend, hip_stream(stream)), who, "launch");
}

// Their backward entry points: prep_gru, then the outputs (the last nout
// operands) must be nout different arrays, then the launch.
int gru_backward(const char *who, void *const *ops, const char *const *names, int nops, int nout,
                 const long *strides, int dtype, int N, int C, long HW, bool blend, void *stream) {
    g_err[0] = 0;
    rc::GruBwdArgs a;
    bool empty;
    if (int rc = prep_gru(who, ops, names, nops, strides, dtype, N, C, HW, a, &empty)) return rc;
    if (empty) return RC_OK;
    for (int i = nops - nout; i < nops; ++i)
        for (int k = i + 1; k < nops; ++k)
            if (ops[i] == ops[k])
                return fail(RC_EINVAL, "%s: %s and %s alias each other (two outputs in one array)", who,
                            names[i], names[k]);
    return hip_rc(rc_launch_gru_bwd(a, dtype, blend, hip_stream(stream)), who, "launch");
}
}  // namespace

extern "C" int rc_gru_gates(const void *z_pre, const void *r_pre, const void *cz, const void *cr,
                            const void *h, void *z_out, void *rh_out, const long *strides, int dtype, int N,
                            int C, long HW, void *stream) {
    void *const ops[7] = {mut(z_pre), mut(r_pre), mut(cz), mut(cr), mut(h), z_out, rh_out};
    const char *const names[7] = {"z_pre", "r_pre", "cz", "cr", "h", "z_out", "rh_out"};
    return gru_forward("rc_gru_gates", ops, names, 7, strides, dtype, N, C, HW, false, stream);
}

extern "C" int rc_gru_blend(const void *z, const void *q_pre, const void *cq, const void *h, void *h_out,
                            const long *strides, int dtype, int N, int C, long HW, void *stream) {
    void *const ops[5] = {mut(z), mut(q_pre), mut(cq), mut(h), h_out};
    const char *const names[5] = {"z", "q_pre", "cq", "h", "h_out"};
    return gru_forward("rc_gru_blend", ops, names, 5, strides, dtype, N, C, HW, true, stream);
}

extern "C" int rc_gru_gates_backward(const void *g_z, const void *g_rh, const void *z, const void *r_pre,
                                     const void *cr, const void *h, void *g_zpre, void *g_rpre, void *g_h,
                                     const long *strides, int dtype, int N, int C, long HW, void *stream) {
    void *const ops[9] = {mut(g_z), mut(g_rh), mut(z), mut(r_pre), mut(cr), mut(h), g_zpre, g_rpre, g_h};
    const char *const names[9] = {"g_z", "g_rh", "z", "r_pre", "cr", "h", "g_zpre", "g_rpre", "g_h"};
    return gru_backward("rc_gru_gates_backward", ops, names, 9, 3, strides, dtype, N, C, HW, false, stream);
}

extern "C" int rc_gru_blend_backward(const void *g_out, const void *z, const void *q_pre, const void *cq,
                                     const void *h, void *g_z, void *g_qpre, void *g_h, const long *strides,
                                     int dtype, int N, int C, long HW, void *stream) {
    void *const ops[8] = {mut(g_out), mut(z), mut(q_pre), mut(cq), mut(h), g_z, g_qpre, g_h};
    const char *const names[8] = {"g_out", "z", "q_pre", "cq", "h", "g_z", "g_qpre", "g_h"};
    return gru_backward("rc_gru_blend_backward", ops, names, 8, 3, strides, dtype, N, C, HW, true, stream);
}

namespace {
// What rc_gru_assemble and rc_gru_assemble_backward check alike, in the steps
// both take in this order; each entry point puts its own checks between them.
// The forward's buffer is dst and its parts the sources, the backward's g and
// the sources' gradients; the nouns of the messages come with the arguments.
// Part is rc::GruPart or rc::GruBwdPart (common.h keeps the two apart).
template <class Part>
struct Assembly {
    using Ptr = decltype(Part::p);
    const char *who, *buf_name, *parts_name, *stem, *of;   // "dst" "src" "src" "" / "g" "grad_src" "grad" " of g"
    const void *buf;
    const long *buf_strides;
    int buf_dtype, N, H, W, nparts;
    Ptr const *parts;
    const long *part_strides;
    const int *part_dtype, *mode, *channels, *src_h, *src_w;
    long long C = 0;    // channels of the parts added so far

    // the null-array ladder, the buffer's element kind, the shape, the buffer's strides
    int arguments() const {
        if (nparts < 1 || nparts > RC_GRU_MAX_PARTS)
            return fail(RC_EINVAL, "%s: nparts=%d outside 1..%d", who, nparts, RC_GRU_MAX_PARTS);
        if (!buf) return fail(RC_EINVAL, "%s: null %s", who, buf_name);
        if (!buf_strides) return fail(RC_EINVAL, "%s: null %s_strides", who, buf_name);
        if (!parts) return fail(RC_EINVAL, "%s: null %s", who, parts_name);
        if (!part_strides) return fail(RC_EINVAL, "%s: null %s_strides", who, stem);
        if (!part_dtype) return fail(RC_EINVAL, "%s: null %s_dtype", who, stem);
        if (!mode) return fail(RC_EINVAL, "%s: null mode", who);
        if (!channels) return fail(RC_EINVAL, "%s: null channels", who);
        if (!src_h || !src_w) return fail(RC_EINVAL, "%s: null %s", who, src_h ? "src_w" : "src_h");
        if (!known_kind(buf_dtype))
            return fail(RC_EINVAL, "%s: unknown %s_dtype %d (RC_F32, RC_F16 or RC_BF16)", who, buf_name, buf_dtype);
        if (N < 0 || H < 0 || W < 0) return fail(RC_EINVAL, "%s: bad shape N=%d H=%d W=%d", who, N, H, W);
        for (int k = 0; k < 4; ++k)
            if (buf_strides[k] < 0)
                return fail(RC_EINVAL, "%s: negative stride in %s_strides (%ld, %ld, %ld, %ld)", who, buf_name,
                            buf_strides[0], buf_strides[1], buf_strides[2], buf_strides[3]);
        return RC_OK;
    }

    // part i: its element kind, mode, channels, strides and size, the size a
    // copied or pooled part must have; then its descriptor P, at channel C
    int add_part(int i, Part &P) {
        const long *t = part_strides + 4 * i;
        const int SH = src_h[i], SW = src_w[i];
        if (!known_kind(part_dtype[i]))
            return fail(RC_EINVAL, "%s: unknown %s_dtype[%d] = %d (RC_F32, RC_F16 or RC_BF16)", who, stem, i,
                        part_dtype[i]);
        if (mode[i] != RC_PART_COPY && mode[i] != RC_PART_POOL2X && mode[i] != RC_PART_BILINEAR)
            return fail(RC_EINVAL, "%s: unknown mode[%d] = %d (RC_PART_COPY, RC_PART_POOL2X or RC_PART_BILINEAR)",
                        who, i, mode[i]);
        if (channels[i] < 1) return fail(RC_EINVAL, "%s: channels[%d] = %d, at least 1", who, i, channels[i]);
        if (t[0] < 0 || t[1] < 0 || t[2] < 0 || t[3] < 0)
            return fail(RC_EINVAL, "%s: negative stride in %s_strides of part %d (%ld, %ld, %ld, %ld)", who, stem, i,
                        t[0], t[1], t[2], t[3]);
        if (SH < 1 || SW < 1)
            return fail(RC_EINVAL, "%s: src_h[%d] x src_w[%d] = %d x %d, at least 1 x 1", who, i, i, SH, SW);
        if (mode[i] == RC_PART_COPY && H && W && (SH != H || SW != W))
            return fail(RC_EINVAL, "%s: RC_PART_COPY part %d has src_h x src_w = %d x %d, %s %d x %d", who, i,
                        SH, SW, buf_name, H, W);
        const int PH = (SH - 1) / 2 + 1, PW = (SW - 1) / 2 + 1;   // 3x3, stride 2, padding 1
        if (mode[i] == RC_PART_POOL2X && H && W && (H != PH || W != PW))
            return fail(RC_EINVAL, "%s: RC_PART_POOL2X part %d has src_h x src_w = %d x %d, which pools to "
                        "%d x %d, %s is %d x %d", who, i, SH, SW, PH, PW, buf_name, H, W);
        P.p = parts[i];
        P.sn = t[0], P.sc = t[1], P.sh = t[2], P.sw = t[3];
        P.c0 = (int)C, P.C = channels[i];
        P.mode = mode[i], P.ek = part_dtype[i];
        P.SH = SH, P.SW = SW;
        P.scale_h = H > 1 ? (float)(SH - 1) / (float)(H - 1) : 0.0f;   // bilinear, align_corners
        P.scale_w = W > 1 ? (float)(SW - 1) / (float)(W - 1) : 0.0f;
        C += channels[i];
        return RC_OK;
    }

    // the buffer's layout class (*planar, else interleaved), then *empty (RC_OK,
    // nothing to do) or the 2^31 - 1 limits of the kernels' indices
    int layout(bool *planar, bool *empty) const {
        const long *t = buf_strides;
        *planar = (W <= 1 || t[3] == 1) && (H <= 1 || t[2] == (long)W * t[3]);
        const bool inter = C == 1 || t[1] == 1;
        if (!*planar && !inter)
            return fail(RC_EUNSUPPORTED, "%s: %s_strides (%ld, %ld, %ld, %ld) are neither planar (column stride 1, "
                        "row stride W) nor interleaved (channel stride 1)", who, buf_name, t[0], t[1], t[2], t[3]);
        *empty = (long long)N * H * W == 0;
        if (*empty) return RC_OK;
        const long long lim = 0x7FFFFFFFLL;
        if ((long long)N * H > lim || (long long)N * H * W > lim || (long long)N * H * W * C > lim)
            return fail(RC_EUNSUPPORTED, "%s: N*C*H*W elements%s (N=%d C=%lld H=%d W=%d) exceed 2^31 - 1", who, of, N,
                        C, H, W);
        return RC_OK;
    }

    // every array on a multiple of its element size (a null one passes): the
    // buffer, `also` (the backward's g2, of the buffer's element kind), the parts
    int aligned(const void *also = nullptr, const char *also_name = nullptr) const {
        const char *bad = !elem_aligned(buf, buf_dtype) ? buf_name : !elem_aligned(also, buf_dtype) ? also_name : nullptr;
        if (bad) return fail(RC_EINVAL, "%s: %s is not aligned to its element size", who, bad);
        for (int i = 0; i < nparts; ++i)
            if (!elem_aligned(parts[i], part_dtype[i]))
                return fail(RC_EINVAL, "%s: %s[%d] is not aligned to its element size", who, parts_name, i);
        return RC_OK;
    }
};
}  // namespace

extern "C" int rc_gru_assemble(void *dst, const long *dst_strides, int dst_dtype, int N, int H, int W, int nparts,
                               const void *const *src, const long *src_strides, const int *src_dtype,
                               const int *mode, const int *channels, const int *src_h, const int *src_w,
                               void *stream) {
    g_err[0] = 0;
    Assembly<rc::GruPart> as{"rc_gru_assemble", "dst", "src", "src", "", dst, dst_strides, dst_dtype, N, H, W, nparts,
                             src, src_strides, src_dtype, mode, channels, src_h, src_w};
    if (int rc = as.arguments()) return rc;
    rc::GruAsmArgs a;
    for (int i = 0; i < rc::kGruMaxParts; ++i) a.part[i] = rc::GruPart{};
    for (int i = 0; i < nparts; ++i) {
        if (!src[i]) return fail(RC_EINVAL, "%s: null src[%d]", as.who, i);
        if (int rc = as.add_part(i, a.part[i])) return rc;
        if (src[i] == dst) return fail(RC_EINVAL, "%s: dst is src[%d] (dst must not alias a source)", as.who, i);
    }
    for (int i = 0; i < rc::kGruMaxParts; ++i) a.cend[i] = i < nparts ? a.part[i].c0 + a.part[i].C : (int)as.C;
    bool planar, empty;
    int rc = as.layout(&planar, &empty);
    if (rc || empty) return rc;
    if ((rc = as.aligned())) return rc;
    a.dst = dst;
    a.dn = dst_strides[0], a.dc = dst_strides[1], a.dh = dst_strides[2], a.dw = dst_strides[3];
    a.N = N, a.C = (int)as.C, a.H = H, a.W = W;
    a.nparts = nparts;
    a.J = a.units = 0;
    return hip_rc(rc_launch_gru_assemble(a, dst_dtype, !planar, hip_stream(stream)), as.who, "launch");
}

extern "C" int rc_gru_assemble_backward(const void *g, const void *g2, int g2_c0, const long *g_strides, int g_dtype,
                                        int N, int H, int W, int nparts, void *const *grad_src,
                                        const long *grad_strides, const int *grad_dtype, const int *mode,
                                        const int *channels, const int *src_h, const int *src_w, void *stream) {
    g_err[0] = 0;
    Assembly<rc::GruBwdPart> as{"rc_gru_assemble_backward", "g", "grad_src", "grad", " of g", g, g_strides, g_dtype, N,
                                H, W, nparts, grad_src, grad_strides, grad_dtype, mode, channels, src_h, src_w};
    const char *who = as.who;
    if (int rc = as.arguments()) return rc;
    if (g2 == g) return fail(RC_EINVAL, "%s: g2 is g (pass the sum's halves as two arrays, or g alone)", who);
    rc::GruAsmBwdArgs a;
    for (int i = 0; i < rc::kGruMaxParts; ++i) a.part[i] = rc::GruBwdPart{};
    long long most = 0;     // elements of the largest output
    int wanted = 0;         // parts with an output (grad_src[i] given)
    for (int i = 0; i < nparts; ++i) {
        if (int rc = as.add_part(i, a.part[i])) return rc;
        a.part[i].J = 1, a.part[i].u0 = 0;
        if (!grad_src[i]) continue;
        ++wanted;
        if (grad_src[i] == g || grad_src[i] == g2)
            return fail(RC_EINVAL, "%s: grad_src[%d] is %s (no output may overlap a gradient it is computed "
                        "from)", who, i, grad_src[i] == g ? "g" : "g2");
        for (int k = 0; k < i; ++k)
            if (grad_src[k] == grad_src[i])
                return fail(RC_EINVAL, "%s: grad_src[%d] is grad_src[%d] (two outputs in one array)", who, i, k);
        most = std::max(most, (long long)N * channels[i] * src_h[i] * src_w[i]);
    }
    if (!wanted) return fail(RC_EINVAL, "%s: every grad_src[i] is null (nothing to compute)", who);
    if (g2_c0 < 0 || g2_c0 > as.C) return fail(RC_EINVAL, "%s: g2_c0=%d outside 0..%lld", who, g2_c0, as.C);
    bool planar, empty;
    int rc = as.layout(&planar, &empty);
    if (rc || empty) return rc;
    if (most > 0x7FFFFFFFLL)
        return fail(RC_EUNSUPPORTED, "%s: an output of %lld elements exceeds 2^31 - 1", who, most);
    if ((rc = as.aligned(g2, "g2"))) return rc;
    a.g = g, a.g2 = g2;
    a.gn = g_strides[0], a.gc = g_strides[1], a.gh = g_strides[2], a.gw = g_strides[3];
    a.g2_c0 = g2_c0;
    a.N = N, a.C = (int)as.C, a.H = H, a.W = W;
    a.nparts = nparts;
    a.units = 0;
    return hip_rc(rc_launch_gru_assemble_bwd(a, g_dtype, !planar, hip_stream(stream)), who, "launch");
}
