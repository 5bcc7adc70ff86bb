"""Dense width sweeps of the per-iteration kernels against the C oracle on
guarded memory: the lookups (rc_corr_lookup, rc_corr_lookup_chain,
rc_corr_lookup_step), the lookups fused with convc1 (rc_corr_lookup_conv,
rc_corr_lookup_chain_conv) and the lookup backwards (rc_corr_lookup_backward,
rc_corr_lookup_backward_calls, rc_corr_lookup_conv_backward,
rc_corr_lookup_chain_conv_backward).

Every call goes through the raw C ABI on arena memory (sweep_util.py,
lookup_sweep_util.py): levels, coordinates and outputs at addresses 16 or 80
mod 128 between 4 KiB guards of a NaN pattern.  Guards and inputs must be
bit-identical after the call and no output element may still hold the pattern.
The pyramids are made on the CPU (lookup_sweep_util.cpu_pyramid: random level
0, the oracle's / numpy's pooling above it), so nothing here depends on the
project's build, except where the layout is a build product (disparity-major
levels, records).  Rows are padded to 16 bytes and the padding, the gap before
a shadow copy and the coordinates' y channel hold the NaN pattern; levels a
kernel is documented not to read are NULL.

Shapes: (B, H, W1) in (1,1,37), (2,1,37), (1,2,70), (2,2,70): P = 37 (a
partial wave), 74 (two waves), 140, 280 (two 256-pixel workgroups, the second
with 24 lanes), rotating with the width.  Coordinates per case: special_coords
(NaN, +-inf, +-1e30, +-0, subnormals, out of range), every integer from -40 to
W2 + 40 with both fp32 neighbours, and one smooth field.

Which case reaches which kernel instance (derived from the dispatch code;
lookup_sweep_util.py restates the computable parts and
test_lookup_sweep_host.py asserts them for these very lists):

rc_corr_lookup_chain (capi.cpp, chain_kind; csrc/lookup.hip, launch_pair_r):
  2 levels, or 4 levels with pyr[2] given: the pair kernel
    lookup_pair_kernel<R, NL, 0, BF16, 1, CL> (csrc/lookup_pair.h), R = radius
    1..4, one pixel per lane, 256 per workgroup; with RC_OUT_F16 / RC_OUT_BF16
    the same body with a 16-bit OT (csrc/lookup_half.hip); an fp16 pyramid:
    lookup_f16pyr_pair_kernel<R, NL, CL, OT> (csrc/lookup_f16pyr.hip).
    Each span is read as 16-byte chunks (4 fp32 / 8 16-bit elements) that start
    inside the row and may end in its 16-byte padding (plan_pair_loads): W2
    16..143 (L = 4) covers every residue of W2 mod 64, so every residue mod 16
    of the level-0 and of the level-2 width, odd widths at all four levels; W2
    4..67 the same for L = 2.  Each 16-bit pyramid type runs at every second
    width, the parity flipping every 32 widths, so it meets every residue of
    W2 mod 32 (level-2 width mod 8 = its chunk).
    RC_SHADOW / RC_SHADOW_LEVEL(2): each lane reads from the copy in which its
    span touches fewer 128-byte lines; the gap between the copies is poisoned.
    RC_OUT_CHANNELS_LAST: a wave's 64 x C outputs are gathered in LDS and go
    out as 16-byte vectors (4 fp32 / 8 16-bit elements); the last vector of a
    partial wave goes out element by element when (P % 64) * C is not a
    multiple of the vector: test_channels_last_tail, P % 64 in {1, 37}, C in
    {6, 10, 14, 18} (L = 2) and {12, 20, 28, 36} (L = 4), giving (P % 64) * C
    = 2, 4, 6 mod 8 and 2 mod 4.
  otherwise 3 or 4 levels with pyr[1] given: lookup_chain_kernel<R, NL, 0>
    (csrc/lookup.hip, launch_chain_m), fp32 only, reads levels 0 and 1.
  RC_LAYOUT_DISPARITY: lookup_sheared_pair_kernel<R, 2 | 4>;
  RC_LAYOUT_RECORDS: lookup_records_kernel<R, CL, 0, true[, 1, OT]>.
rc_corr_lookup (csrc/lookup.hip, launch_r), fp32 / bf16 levels:
    P < 65,536 and L <= 4: lookup_levelpar_kernel<R, BF16>, one wave per (64
      pixels, level) -- every small case of L = 1..4;
    else P < 131,072 and L in {3, 4}: lookup_kernel<R, NL, BF16, true, 64>, every
      level's loads up front, 64-thread blocks -- P = 65,590 (H = 937, W1 = 70);
    else lookup_kernel<R, 0, BF16, true>, the runtime level loop, 256 threads --
      P = 131,110 (H = 1873), and every case of L = 5.
  fp16 levels: lookup_f16pyr_level_kernel<R> at any P.
rc_corr_lookup_step, chain != 0: the chain kernels above with the coordinate
  update in front (pixel_x, csrc/lookup_level.h).
rc_corr_lookup_conv: lookup_conv_kernel<R, NL, BF16> (NL = 2..4);
rc_corr_lookup_chain_conv: lookup_pair_conv_kernel<R, NL, BF16, OT>.
rc_corr_lookup_backward (csrc/backward.hip, rc_launch_lookup_bwd): grad_pyr[1]
  NULL: lookup_bwd_pair_kernel<R, 2 | 4>; else lookup_bwd_pre_kernel<R, NL>.
rc_corr_lookup_backward_calls (csrc/backward_calls.hip): the pair layout at
  these widths: lookup_bwd_calls_compact_kernel<R, 2 | 4>, one launch per 32
  calls (33 calls: two launches, the second accumulating).
rc_corr_lookup_conv_backward / _chain_conv_backward: lookup_conv_bwd_kernel /
  lookup_pair_conv_grad_kernel, one partial sum per 256-pixel workgroup (P =
  37, 256, 257, 513: 1, 1, 2, 3 workgroups), then lookup_conv_bwd_reduce_kernel.

A looked-up level of width 1 (the C ABI accepts it; the reference cannot
reach it): the sampler divides by W - 1 = 0 and the reference's arithmetic is
NaN for every tap at every x.  The kernels give the same NaNs, also where
they short-cut a far-away x to "every tap is zero padding", because the tap
weights are NaN too (test_width_one_level; include/raftcorr.h).

Bounds:
  lookups: bit for bit against coracle.corr_lookup on the CPU pyramid (NaN
    positions coincide, every other element has the same bits); 16-bit outputs
    against ``.to(dtype)`` of the oracle's fp32 result, the rule of
    test_out_dtype_gpu.py;
  fused conv: rc_corr_lookup_conv <= 1e-5 normalised against an fp64 conv of
    the oracle's lookup (test_corr_gpu.test_lookup_convc1_vs_separate); the
    chain kernel's fp32 output bit-equal to it (include/raftcorr.h), 16-bit
    outputs bit-equal to ``.to(dtype)`` of the kernel's own fp32 output;
  lookup backward: <= 1e-6 normalised against coracle.corr_lookup_backward
    (test_backward.test_lookup_backward_levels_vs_oracle).  The buffers start
    from 0.25 x randn and the kernel adds to them, so what is compared is the
    buffer against initial contents + oracle, normalised by the largest
    magnitude of that sum (as test_backward_calls_gpu.py does for its
    accumulate mode): an fp32 ``+=`` cannot keep a contribution below half an
    ulp of what the buffer holds, so the difference to the initial contents
    normalised by max|oracle| alone has no bound where a level's whole
    gradient is tiny (an x sweep that lies outside the row gives weights of
    1e-7: measured 1.0 there);
  backward_calls: <= 1e-6 (norm_err and rel-L2) against the oracle and <= 1e-6
    against the per-call kernel (test_backward_calls_gpu.py);
  conv backward: <= 1e-5 normalised against fp64 on the oracle's lookup
    (test_convc1_backward_gpu.py; grad_out zeroed at the reference's ReLU
    kinks as there, the kink band being the rounding error bound of the
    kernel's fp32 chain); the chain variant bit-equal to the per-level one.
Each test prints the largest error it saw against its bound.
"""
import numpy as np
import pytest
import torch

import lookup_sweep_util as lsu
import sweep_util as su
from golden_util import norm_err, rel_l2
from oracle import coracle
from raft_stereo_amd import _lib
from raft_stereo_amd import corr as rcorr
from test_out_dtype_gpu import assert_same_half
from test_volume_sweep_gpu import Worst, band_id, fmaps

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF16 = torch.bfloat16
CL, O16, OB16 = _lib.RC_OUT_CHANNELS_LAST, _lib.RC_OUT_F16, _lib.RC_OUT_BF16
CONV_TOL, BWD_TOL, CALLS_TOL, CONV_BWD_TOL = 1e-5, 1e-6, 1e-6, 1e-5

# name -> (output flags, shadowed levels)
PAIR_FLAGS = {"none": (0, ()), "shadow": (0, "all"), "shadow2": (0, (2,)), "cl": (CL, ()), "f16": (O16, ()),
              "bf16": (OB16, ()), "cl_f16": (CL | O16, ()), "cl_bf16": (CL | OB16, ())}
assert list(PAIR_FLAGS) == lsu.PAIR_FLAG_NAMES


def bit_same(a, b):
    """NaN positions coincide and every other element has the same bits."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and \
        np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


def check_lookups(outs, pyr, xs, L, r, flags, tag):
    out_dt = lsu.OUT_DT.get(flags & lsu.OUT_HALF)
    for k, (got, x) in enumerate(zip(outs, xs)):
        ref = coracle.corr_lookup(pyr, lsu.as_coords(x), L, r)
        if out_dt is None:
            if not bit_same(got, ref):
                got = np.ascontiguousarray(got, np.float32)
                bad = np.argwhere(~((got.view(np.uint32) == ref.view(np.uint32)) | (np.isnan(got) & np.isnan(ref))))
                b, c, h, w = bad[0]
                raise AssertionError(f"{tag} coords {k}: {len(bad)} elements differ, the first at (b, c, h, w) = "
                                     f"{(b, c, h, w)}: x = {x[b, h, w]!r}, got {got[b, c, h, w]!r}, "
                                     f"oracle {ref[b, c, h, w]!r}")
        else:
            assert_same_half(got, torch.from_numpy(ref), out_dt, f"{tag} coords {k}")


def pair_stored(L):
    return (0, 2) if L == 4 else (0,)


def pair_case(W2, L, r, kind, fname, i):
    """One pair-kernel lookup case (part a)."""
    flags, shadow = PAIR_FLAGS[fname]
    B, H, W1 = lsu.shape_for(i)
    bf = kind != "f32" or bool(flags & lsu.OUT_HALF)
    pyr = lsu.cpu_pyramid(B * H * W1, W2, L, kind, 7 * W2 + L)
    lv = lsu.Levels.rows(pyr, kind, pair_stored(L), shadow, bf)
    xs = lsu.all_sets(lsu.coord_sets(B, H, W1, W2, W2 + r))
    outs = lsu.guarded_lookup(DEV, "rc_corr_lookup_chain", lv, L, r, xs, flags, phase=i + r, bf=bf)
    check_lookups(outs, pyr, xs, L, r, flags, f"pair {kind} {fname} L={L} r={r} W2={W2} shape={(B, H, W1)}")


# ----------------------------------------------------------- a. pair kernel

@pytest.mark.parametrize("fname", lsu.PAIR_FLAG_NAMES)
@pytest.mark.parametrize("band", lsu.PAIR_BANDS[4], ids=band_id)
def test_pair_lookup_4_levels(band, fname):
    for W2 in band:
        for kind in lsu.pair_kinds(W2):
            for r in lsu.pair_radii(W2, 4):
                pair_case(W2, 4, r, kind, fname, W2)


@pytest.mark.parametrize("fname", [f for f in lsu.PAIR_FLAG_NAMES if f != "shadow2"])
@pytest.mark.parametrize("band", lsu.PAIR_BANDS[2], ids=band_id)
def test_pair_lookup_2_levels(band, fname):
    for W2 in band:
        for kind in lsu.pair_kinds(W2):
            for r in lsu.pair_radii(W2, 2):
                pair_case(W2, 2, r, kind, fname, W2)


@pytest.mark.parametrize("kind", lsu.KINDS)
@pytest.mark.parametrize("L", [2, 4])
def test_channels_last_tail(L, kind):
    """The last vector of a partial wave's channels-last run, element by
    element: P % 64 in {1, 37}, every C of the level count, fp32 outputs
    (vectors of 4) and 16-bit outputs (vectors of 8)."""
    W2 = lsu.CL_TAIL_W2[L]
    for W1 in lsu.CL_TAIL_W1:
        for r in (1, 2, 3, 4):
            for out in (0, O16, OB16):
                flags = CL | out
                bf = kind != "f32" or bool(out)
                pyr = lsu.cpu_pyramid(W1, W2, L, kind, W1 + r)
                lv = lsu.Levels.rows(pyr, kind, pair_stored(L), (), bf)
                cs = lsu.coord_sets(1, 1, W1, W2, W1 + r)
                xs = cs["special"] + cs["smooth"]
                outs = lsu.guarded_lookup(DEV, "rc_corr_lookup_chain", lv, L, r, xs, flags, phase=r, bf=bf)
                check_lookups(outs, pyr, xs, L, r, flags, f"cl tail {kind} L={L} r={r} W1={W1} out={out:#x}")


# -------------------------------------------------- b. level-1 chain kernel

@pytest.mark.parametrize("L", [3, 4])
@pytest.mark.parametrize("band", [0, 1, 2, 3])
def test_level1_chain_lookup(band, L):
    """pyr[1] given, pyr[2] (and pyr[3]) NULL: lookup_chain_kernel."""
    for W2 in lsu.CHAIN_W2[L][16 * band:16 * band + 16]:
        for r in (1, 4):
            B, H, W1 = lsu.shape_for(W2)
            pyr = lsu.cpu_pyramid(B * H * W1, W2, L, "f32", 5 * W2 + L)
            lv = lsu.Levels.rows(pyr, "f32", (0, 1))
            xs = lsu.all_sets(lsu.coord_sets(B, H, W1, W2, W2 + r))
            outs = lsu.guarded_lookup(DEV, "rc_corr_lookup_chain", lv, L, r, xs, phase=W2 + r)
            check_lookups(outs, pyr, xs, L, r, 0, f"level-1 chain L={L} r={r} W2={W2}")


# -------------------------------------------------------- c. per-level

@pytest.mark.parametrize("kind", lsu.KINDS)
@pytest.mark.parametrize("L", [1, 2, 3, 4, 5])
def test_per_level_lookup(L, kind):
    for i, W2 in enumerate(lsu.level_w2(L)):
        for r in (1, 4, 8):
            B, H, W1 = lsu.shape_for(i)
            bf = kind != "f32"
            pyr = lsu.cpu_pyramid(B * H * W1, W2, L, kind, 3 * W2 + L)
            lv = lsu.Levels.rows(pyr, kind, None, (), bf)
            xs = lsu.all_sets(lsu.coord_sets(B, H, W1, W2, W2 + r))
            outs = lsu.guarded_lookup(DEV, "rc_corr_lookup", lv, L, r, xs, phase=i + r, bf=bf)
            check_lookups(outs, pyr, xs, L, r, 0, f"per-level {kind} L={L} r={r} W2={W2}")


@pytest.mark.parametrize("shape", lsu.LARGE_P, ids=lambda s: f"P{s[0] * s[1] * s[2]}")
def test_per_level_lookup_large_p(shape):
    """P just above 65,536: the 64-thread unrolled kernel; just above 131,072:
    the runtime-loop kernel (W2 = 16, L = 4, r = 4)."""
    B, H, W1 = shape
    W2, L, r = 16, 4, 4
    assert lsu.level_kernel(B * H * W1, L, "f32") == ("unrolled64" if H < 1000 else "runtime_loop")
    pyr = lsu.cpu_pyramid(B * H * W1, W2, L, "f32", H)
    lv = lsu.Levels.rows(pyr, "f32")
    xs = [lsu.packed_coords(B, H, W1, W2, H)]
    outs = lsu.guarded_lookup(DEV, "rc_corr_lookup", lv, L, r, xs, phase=H)
    check_lookups(outs, pyr, xs, L, r, 0, f"per-level P={B * H * W1}")


# ------------------------------------------------------ d. disparity-major

@pytest.mark.parametrize("L", [2, 4])
def test_disparity_major_lookup(L):
    """RC_LAYOUT_DISPARITY: the levels are a build product (su.guarded_sheared);
    the reference is the oracle on unshear_level of them.  Entries outside the
    rows' widths keep the build arena's NaN pattern."""
    for i, (W1, W2) in enumerate(lsu.DISP_LOOKUP):
        f1, f2 = fmaps(su.F32_D, 1, W1, W2, 3 * W1 + W2)
        _, S = su.guarded_sheared(DEV, f1, f2, L, phase=i)
        keep = sorted(S)
        flat = {l: rcorr.unshear_level(S[l], l, 1, 1, W1, W2).reshape(W1, -1).cpu().numpy() for l in keep}
        pyr = []
        for l in keep:
            assert np.isfinite(flat[l]).all()
            pyr += [flat[l], coracle.corr_pool(flat[l])]
        ld = su.grad_ld(W1)
        cpu = {l: S[l].cpu() for l in keep}
        lv = lsu.Levels([(f"s{l}", cpu[l].numel() * 4, cpu[l]) for l in keep],
                        [f"s{l}" if l in keep else None for l in range(L)], [W2 >> l for l in range(L)],
                        [ld if l in keep else W2 >> l for l in range(L)], _lib.RC_F32 | _lib.RC_LAYOUT_DISPARITY)
        xs = lsu.all_sets(lsu.coord_sets(1, 1, W1, W2, W1 + W2))
        for r in (1, 4):
            outs = lsu.guarded_lookup(DEV, "rc_corr_lookup_chain", lv, L, r, xs, _lib.RC_LAYOUT_DISPARITY, phase=i + r)
            check_lookups(outs, pyr, xs, L, r, 0, f"disparity-major L={L} r={r} W1={W1} W2={W2}")


# --------------------------------------------------------------- e. records

def record_levels(W2, W1, seed, phase):
    """Records from su.guarded_records (bf16 fmaps, D = 225), as a CPU tensor,
    and the four levels they hold."""
    f1, f2 = fmaps(225, 1, W1, W2, seed, BF16)
    _, rec = su.guarded_records(DEV, f1, f2, phase=phase)
    lv = {l: rcorr.records_level(rec, l, W2).reshape(W1, -1).float().cpu().numpy() for l in (0, 2)}
    pyr = [lv[0], su.bf16_pool_np(lv[0]), lv[2], su.bf16_pool_np(lv[2])]
    cpu = rec.cpu().contiguous()
    levels = lsu.Levels([("rec", cpu.numel() * 2, cpu)], ["rec", None, None, None], [W2 >> l for l in range(4)],
                        None, _lib.RC_BF16 | _lib.RC_LAYOUT_RECORDS)
    return levels, pyr


@pytest.mark.parametrize("W2", lsu.REC_LOOKUP_W2)
def test_records_lookup(W2):
    """RC_LAYOUT_RECORDS with the lookup output inside the arena, NCHW and
    channels-last, fp32 and both 16-bit types."""
    W1 = 70
    lv, pyr = record_levels(W2, W1, W2, W2)
    xs = lsu.all_sets(lsu.coord_sets(1, 1, W1, W2, W2))
    for r in (1, 4):
        for flags in (0, CL, O16, OB16, CL | O16, CL | OB16):
            outs = lsu.guarded_lookup(DEV, "rc_corr_lookup_chain", lv, 4, r, xs, _lib.RC_LAYOUT_RECORDS | flags,
                                      phase=r, bf=True)
            check_lookups(outs, pyr, xs, 4, r, flags, f"records r={r} W2={W2} flags={flags:#x}")


# ------------------------------------------------------------------ f. step

def step_case(lv, pyr, W2, B, H, W1, r, with_delta, alias, bf, extra, tag, phase):
    cs = lsu.coord_sets(B, H, W1, W2, W2 + r)
    g = torch.Generator().manual_seed(W2 + r)
    for k, x in enumerate(lsu.all_sets(cs)):
        c0 = lsu.coords_grid(B, H, W1)
        c1 = c0.clone()
        c1[:, 0] = torch.from_numpy(x)
        c1[:, 1] += 0.25                                   # y finite, flow_y = 0.25
        dx = (torch.randn(B, H, W1, generator=g) * 3).numpy() if with_delta else None
        out, c1_out, flow = lsu.guarded_step(DEV, lv, 4, r, c1, dx, alias, extra, phase=phase + k, bf=bf)
        want = c1.clone()
        if with_delta:
            d = torch.zeros(B, 2, H, W1)
            d[:, 0] = torch.from_numpy(dx)                  # delta_flow[:, 1] = 0
            want = want + d
        assert bit_same(c1_out, want.numpy()), f"{tag} coords {k}: coords1_out"
        assert bit_same(flow, (want - c0).numpy()), f"{tag} coords {k}: flow_out"
        assert np.isfinite(c1_out[:, 1]).all() and np.isfinite(flow[:, 1]).all(), f"{tag}: delta's y reached y"
        check_lookups([out], pyr, [want[:, 0].numpy()], 4, r, 0, f"{tag} coords {k}")


@pytest.mark.parametrize("alias", [True, False], ids=["inplace", "separate"])
@pytest.mark.parametrize("with_delta", [False, True], ids=["nodelta", "delta"])
@pytest.mark.parametrize("layout", ["pair_f32", "pair_bf16", "records"])
def test_lookup_step(layout, with_delta, alias):
    """rc_corr_lookup_step, chain != 0: out bit for bit the oracle's at the
    updated coordinates, coords1_out and flow_out bitwise the torch ops';
    delta's y channel is the NaN pattern and must not reach coords1_out[:, 1]."""
    for i, W2 in enumerate(lsu.REC_LOOKUP_W2 if layout == "records" else lsu.STEP_W2):
        r = (1, 4)[i % 2]
        if layout == "records":
            B, H, W1 = 1, 1, 70
            lv, pyr = record_levels(W2, W1, W2 + 1, i)
            bf, extra = True, _lib.RC_LAYOUT_RECORDS
        else:
            B, H, W1 = lsu.shape_for(i)
            kind = layout[5:]
            bf, extra = kind != "f32", 0
            pyr = lsu.cpu_pyramid(B * H * W1, W2, 4, kind, W2)
            lv = lsu.Levels.rows(pyr, kind, (0, 2), (), bf)
        step_case(lv, pyr, W2, B, H, W1, r, with_delta, alias, bf, extra, f"step {layout} r={r} W2={W2}", i)


# -------------------------------------------------------- g. width-1 level

@pytest.mark.parametrize("L,W2", [(4, 8), (4, 15), (2, 2), (2, 3), (3, 4), (3, 7)])
def test_width_one_level(L, W2):
    """Level L - 1 has width 1: the sampler divides by W - 1 = 0 and the
    oracle (the reference's arithmetic) gives NaN for every tap of that level
    at every x -- +-100 and +-1e30, where the kernels short-cut to "every tap
    is zero padding", included.  The kernels reproduce it (the tap weights are
    NaN, so NaN * 0 = NaN): the smallest case of parts a, b, c and f, bit for
    bit against the oracle (include/raftcorr.h, rc_corr_lookup)."""
    B, H, W1 = 1, 1, 37
    x = np.resize(np.array([100, -100, 1e30, -1e30, np.inf, -np.inf, np.nan, 0.0, -0.0, 0.5, 1.0, W2 - 1.0, 2.25],
                           np.float32), W1).reshape(B, H, W1)
    xs = [x] + lsu.coord_sets(B, H, W1, W2, W2)["special"]
    for r in (1, 4):
        T = 2 * r + 1
        pyr = lsu.cpu_pyramid(W1, W2, L, "f32", W2)
        assert pyr[-1].shape[1] == 1
        for xx in xs:                                                # what the oracle says
            ref = coracle.corr_lookup(pyr, lsu.as_coords(xx), L, r)
            assert np.isnan(ref[:, (L - 1) * T:]).all()
        tag = f"width-1 level L={L} W2={W2} r={r}"
        full = lsu.Levels.rows(pyr, "f32")
        outs = lsu.guarded_lookup(DEV, "rc_corr_lookup", full, L, r, xs, phase=r)                        # c
        check_lookups(outs, pyr, xs, L, r, 0, f"{tag} per-level")
        for kind in ("bf16", "f16"):
            p16 = lsu.cpu_pyramid(W1, W2, L, kind, W2)
            outs = lsu.guarded_lookup(DEV, "rc_corr_lookup", lsu.Levels.rows(p16, kind, None, (), True), L, r, xs,
                                      bf=True)
            check_lookups(outs, p16, xs, L, r, 0, f"{tag} per-level {kind}")
        if L != 3:                                                                                       # a
            for fname in ("none", "shadow", "cl", "cl_f16", "bf16"):
                flags, shadow = PAIR_FLAGS[fname]
                for kind in lsu.KINDS:
                    bf = kind != "f32" or bool(flags & lsu.OUT_HALF)
                    pk = lsu.cpu_pyramid(W1, W2, L, kind, W2)
                    lv = lsu.Levels.rows(pk, kind, pair_stored(L), shadow, bf)
                    outs = lsu.guarded_lookup(DEV, "rc_corr_lookup_chain", lv, L, r, xs, flags, phase=r, bf=bf)
                    check_lookups(outs, pk, xs, L, r, flags, f"{tag} pair {kind} {fname}")
        if L >= 3:                                                                                       # b
            chain = lsu.Levels.rows(pyr, "f32", (0, 1))
            outs = lsu.guarded_lookup(DEV, "rc_corr_lookup_chain", chain, L, r, xs, phase=r + 1)
            check_lookups(outs, pyr, xs, L, r, 0, f"{tag} level-1 chain")
        if L == 4:                                                                                       # f
            for kind in ("f32", "bf16"):
                pk = lsu.cpu_pyramid(W1, W2, L, kind, W2)
                lv = lsu.Levels.rows(pk, kind, (0, 2), (), kind != "f32")
                for xx in xs:
                    c1 = lsu.coords_grid(B, H, W1)
                    c1[:, 0] = torch.from_numpy(xx)
                    out, c1_out, _ = lsu.guarded_step(DEV, lv, L, r, c1, None, True, bf=kind != "f32")
                    assert bit_same(c1_out, c1.numpy())
                    check_lookups([out], pk, [xx], L, r, 0, f"{tag} step {kind}")


# ------------------------------------------------------------ h. fused conv

def conv_params(cout, cin, bias, seed):
    g = torch.Generator().manual_seed(seed)
    W = (torch.randn(cout, cin, generator=g) / cin ** 0.5).numpy()
    b = (torch.randn(cout, generator=g) * 0.1).numpy() if bias else None
    return W, b


def conv_ref(pyr, x, L, r, W, b, relu):
    """fp64 ``bias + W @ corr`` on the oracle's lookup."""
    corr = coracle.corr_lookup(pyr, lsu.as_coords(x), L, r).astype(np.float64)
    out = np.einsum("ck,bkhw->bchw", W.astype(np.float64), corr)
    if b is not None:
        out += b.astype(np.float64)[None, :, None, None]
    return np.maximum(out, 0.0) if relu else out


@pytest.mark.parametrize("kind", ["f32", "bf16"])
@pytest.mark.parametrize("L", [2, 3, 4])
def test_lookup_conv(L, kind):
    """rc_corr_lookup_conv on the full CPU pyramid against the fp64 conv of the
    oracle's lookup (finite coordinates); rc_corr_lookup_chain_conv on the pair
    layout (L = 2, 4; plain and RC_SHADOW) bit-equal to it at the special
    coordinates too, and its 16-bit outputs bit-equal to ``.to(dtype)`` of its
    own fp32 output."""
    worst = Worst(f"lookup+convc1 L={L} {kind}")
    bf = kind != "f32"
    combos = [(cout, bias, relu) for cout in (1, 3, 64) for bias in (True, False) for relu in (0, 1)]
    for i, W2 in enumerate(lsu.CONV_W2):
        B, H, W1 = lsu.shape_for(i)
        pyr = lsu.cpu_pyramid(B * H * W1, W2, L, kind, W2 + L)
        cs = lsu.coord_sets(B, H, W1, W2, W2)
        fin, xs = lsu.finite_sets(cs), lsu.all_sets(cs)
        for j, (cout, bias, relu) in enumerate(combos):
            r = 1 + (i + j) % 4
            tag = f"W2={W2} r={r} cout={cout} bias={bias} relu={relu}"
            W, b = conv_params(cout, L * (2 * r + 1), bias, W2 + j)
            full = lsu.Levels.rows(pyr, kind, None, (), bf)
            outs = lsu.guarded_conv(DEV, "rc_corr_lookup_conv", full, L, r, xs, W, b, relu, phase=i + j, bf=bf)
            for x, got in zip(xs, outs):
                if any(x is f for f in fin):
                    worst.add("norm_err", norm_err(got, conv_ref(pyr, x, L, r, W, b, relu)), CONV_TOL, tag)
            if L == 3:
                continue
            for shadow in ((), "all"):
                lv = lsu.Levels.rows(pyr, kind, pair_stored(L), shadow, bf)
                pouts = lsu.guarded_conv(DEV, "rc_corr_lookup_chain_conv", lv, L, r, xs, W, b, relu, phase=j, bf=bf)
                for k, (a, c) in enumerate(zip(pouts, outs)):
                    assert bit_same(a, c), f"{tag} shadow={shadow!r} coords {k}: chain conv != per-level conv"
            dt_flag = (O16, OB16)[(i + j) % 2]
            lv = lsu.Levels.rows(pyr, kind, pair_stored(L), ("all", ())[j % 2], True)
            houts = lsu.guarded_conv(DEV, "rc_corr_lookup_chain_conv", lv, L, r, xs, W, b, relu, dt_flag, phase=i,
                                     bf=True)
            for k, (hgot, c) in enumerate(zip(houts, pouts)):
                assert_same_half(hgot, torch.from_numpy(c), lsu.OUT_DT[dt_flag], f"{tag} coords {k}")
    worst.report()


# ------------------------------------------------------- i. lookup backward

def rand_gouts(n, B, C, H, W1, g):
    return [torch.randn(B, C, H, W1, generator=g).numpy() for _ in range(n)]


def rand_inits(n, P, widths, present, g):
    """0.25 x randn in the whole padded buffer (the padding is never written)."""
    return [{l: (torch.randn(P, su.grad_ld(widths[l]), generator=g) * 0.25).numpy() for l in present}
            for _ in range(n)]


def pair_fold(ref, L):
    """The oracle's per-level gradients folded into the pair layout, as
    test_backward_calls_gpu.oracle_pair: g_e + avg_pool2d backward of g_{e+1}."""
    out = {}
    for e in range(0, L, 2):
        want = np.array(ref[e], dtype=np.float64)
        half = np.repeat(np.asarray(ref[e + 1], np.float64) * 0.5, 2, axis=1)
        want[:, :half.shape[1]] += half
        out[e] = want
    return out


BWD_LAYOUTS = [("level", 1, ()), ("level", 2, ()), ("level", 3, ()), ("level", 4, ()), ("pair", 2, ()),
               ("pair", 4, ()), ("pair", 4, (0,)), ("pair", 4, (2,))]


@pytest.mark.parametrize("layout", BWD_LAYOUTS, ids=lambda t: f"{t[0]}{t[1]}" + "".join(f"_shadow{s}" for s in t[2]))
def test_lookup_backward(layout):
    """rc_corr_lookup_backward into buffers that start from random data, rows
    of stride grad_ld(W): the sums added, the padding and (with a shadow copy)
    the gap unchanged."""
    form, L, shadow = layout
    worst = Worst(f"lookup backward {form} L={L} shadow={shadow}")
    for i, W2 in enumerate(lsu.BWD_W2):
        for r in (1, 4):
            B, H, W1 = lsu.shape_for(i)
            P, C = B * H * W1, L * (2 * r + 1)
            widths = [W2 >> l for l in range(L)]
            present = tuple(range(0, L, 2)) if form == "pair" else tuple(range(L))
            xs = lsu.all_sets(lsu.coord_sets(B, H, W1, W2, W2 + r))
            g = torch.Generator().manual_seed(W2 + r + L)
            gouts = rand_gouts(len(xs), B, C, H, W1, g)
            inits = rand_inits(len(xs), P, widths, present, g)
            gots = lsu.guarded_lookup_backward(DEV, widths, present, L, r, xs, gouts, inits, shadow, phase=i + r)
            for k, (x, go, init, got) in enumerate(zip(xs, gouts, inits, gots)):
                ref = coracle.corr_lookup_backward(widths, lsu.as_coords(x), go, L, r)
                ref = pair_fold(ref, L) if form == "pair" else dict(enumerate(ref))
                for l in present:
                    W = widths[l]
                    tag = f"W2={W2} r={r} coords {k} level {l}"
                    assert np.array_equal(got[l][:, W:], init[l][:, W:].astype(np.float64)), f"{tag}: padding"
                    worst.add("norm_err", norm_err(got[l][:, :W], init[l][:, :W].astype(np.float64) + ref[l]),
                              BWD_TOL, tag)
    worst.report()


# ------------------------------------------------------- j. backward_calls

@pytest.mark.parametrize("mode", ["overwrite", "accumulate"])
@pytest.mark.parametrize("n_calls", [1, 5, 33])
@pytest.mark.parametrize("L", [2, 4])
def test_lookup_backward_calls(L, n_calls, mode):
    """Overwrite mode: the buffers start as the NaN pattern, every row and its
    padding is written, the padding as +0.  Both modes against the oracle
    folded into the pair layout and against n_calls per-call launches."""
    worst = Worst(f"backward_calls L={L} n={n_calls} {mode}")
    present = tuple(range(0, L, 2))
    for i, W2 in enumerate(lsu.CALLS_W2):
        for r in (1, 4):
            B, H, W1 = lsu.shape_for(i)
            P, C = B * H * W1, L * (2 * r + 1)
            widths = [W2 >> l for l in range(L)]
            sets = lsu.all_sets(lsu.coord_sets(B, H, W1, W2, W2 + r))
            xs = [sets[(i + k) % len(sets)] for k in range(n_calls)]
            g = torch.Generator().manual_seed(W2 + r + n_calls)
            gouts = rand_gouts(n_calls, B, C, H, W1, g)
            init = rand_inits(1, P, widths, present, g)[0] if mode == "accumulate" else None
            got = lsu.guarded_lookup_backward_calls(DEV, widths, L, r, xs, gouts, init, phase=i + r)
            zero = {l: np.zeros((P, su.grad_ld(widths[l])), np.float32) for l in present}
            per_call = lsu.guarded_lookup_backward(DEV, widths, present, L, r, xs, gouts, [zero], phase=i,
                                                   chain=True)[0]
            ref = None
            for x, go in zip(xs, gouts):
                ref = coracle.corr_lookup_backward(widths, lsu.as_coords(x), go, L, r, ref)
            want = pair_fold(ref, L)
            for l in present:
                W = widths[l]
                tag = f"W2={W2} r={r} level {l}"
                if init is None:
                    assert not got[l][:, W:].view(np.uint32).any(), f"{tag}: padding not +0"
                    base = 0.0
                else:
                    assert np.array_equal(got[l][:, W:].view(np.uint32), init[l][:, W:].view(np.uint32)), \
                        f"{tag}: padding changed"
                    base = init[l][:, :W].astype(np.float64)
                worst.add("norm_err vs oracle", norm_err(got[l][:, :W], want[l] + base), CALLS_TOL, tag)
                worst.add("rel_l2 vs oracle", rel_l2(got[l][:, :W], want[l] + base), CALLS_TOL, tag)
                worst.add("norm_err vs per-call", norm_err(got[l][:, :W], per_call[l][:, :W] + base), CALLS_TOL, tag)
    worst.report()


# -------------------------------------------------------- k. conv backward

WANTS = [w for m in range(1, 8) for w in [tuple(n for b, n in enumerate(lsu.CONV_BWD_OUTS) if m >> b & 1)]]


def conv_bwd_ref(pyr, x, L, r, W, b, relu, gout):
    """fp64 gradients on the oracle's lookup; returns them and grad_out zeroed
    at the reference's ReLU kinks (decided from the reference alone, as in
    test_convc1_backward_gpu.py; the band is the fp32 chain's error bound)."""
    corr = coracle.corr_lookup(pyr, lsu.as_coords(x), L, r).astype(np.float64)
    pre = np.einsum("ck,bkhw->bchw", W.astype(np.float64), corr)
    if b is not None:
        pre += b.astype(np.float64)[None, :, None, None]
    gout = gout.copy()
    if relu:
        # the kernel's fp32 chain (bias, then one fmaf per k) differs from this
        # fp64 pre by less than (cin + 1) 2^-23 (|b| + sum_k |w_k| |corr_k|): only
        # a pre-activation inside that band can land on the other side of zero
        mag = np.einsum("ck,bkhw->bchw", np.abs(W).astype(np.float64), np.abs(corr))
        if b is not None:
            mag += np.abs(b).astype(np.float64)[None, :, None, None]
        kink = np.abs(pre) < (W.shape[1] + 1) * 2.0 ** -23 * mag
        assert kink.sum() <= max(2, 1e-3 * kink.size), "kink mask touched more than 0.1 % of grad_out"
        gout[kink] = 0.0
    gm = gout.astype(np.float64) * ((pre > 0) if relu else 1.0)
    return {"grad_corr": np.einsum("ck,bchw->bkhw", W.astype(np.float64), gm),
            "grad_weight": np.einsum("bchw,bkhw->ck", gm, corr), "grad_bias": gm.sum((0, 2, 3))}, gout


@pytest.mark.parametrize("shape", lsu.CONV_BWD_P, ids=lambda s: f"P{s[0] * s[1] * s[2]}")
@pytest.mark.parametrize("L", [2, 3, 4])
def test_lookup_conv_backward(L, shape):
    """Every legal combination of NULL outputs, cout in {1, 3, 64}, the
    workspace exactly RC_LOOKUP_CONV_BWD_WS floats between guards; the chain
    variant (L = 2, 4) bit-equal to the per-level one."""
    worst = Worst(f"conv backward L={L} P={shape[0] * shape[1] * shape[2]}")
    B, H, W1 = shape
    n = 0
    for cout in (1, 3, 64):
        for want in WANTS:
            n += 1
            W2 = lsu.CONV_W2[n % len(lsu.CONV_W2)]
            r, relu, bias, kind = 1 + n % 4, n % 2, n % 3 != 0, ("f32", "bf16")[n // 2 % 2]
            tag = f"W2={W2} r={r} cout={cout} {kind} relu={relu} bias={bias} want={want}"
            bf = kind != "f32"
            pyr = lsu.cpu_pyramid(B * H * W1, W2, L, kind, W2 + n)
            x = lsu.finite_sets(lsu.coord_sets(B, H, W1, W2, n))[-1 - n % 2]
            Wt, b = conv_params(cout, L * (2 * r + 1), bias, n)
            g = torch.Generator().manual_seed(n)
            ref, gout = conv_bwd_ref(pyr, x, L, r, Wt, b, relu, torch.randn(B, cout, H, W1, generator=g).numpy())
            full = lsu.Levels.rows(pyr, kind, None, (), bf)
            got = lsu.guarded_conv_backward(DEV, "rc_corr_lookup_conv_backward", full, L, r, x, Wt, b, relu, gout,
                                            want, phase=n)
            for name in want:
                worst.add(f"{name} norm_err", norm_err(got[name], ref[name]), CONV_BWD_TOL, tag)
            if L == 3:
                continue
            lv = lsu.Levels.rows(pyr, kind, pair_stored(L), ("all", ())[n % 2], bf)
            pgot = lsu.guarded_conv_backward(DEV, "rc_corr_lookup_chain_conv_backward", lv, L, r, x, Wt, b, relu,
                                             gout, want, phase=n + 1)
            for name in want:
                assert bit_same(pgot[name], got[name]), f"{tag}: chain {name} != per-level"
    worst.report()
