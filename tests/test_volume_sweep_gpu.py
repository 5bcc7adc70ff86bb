"""Dense width / depth sweeps of the volume kernels against the C oracle:
rc_corr_build in its split-bf16, exact-fp32, bf16 per-wave, bf16 ring, records
and disparity forms, and rc_corr_build_backward.  Every call runs on guarded
arena memory (sweep_util.py): operands and outputs at addresses 16 or 80 mod
128 between 4 KiB guards of a NaN pattern; guards and inputs must be
bit-identical after the call and every output finite.

Which widths reach which kernel instance today (B = 1; derived from the
dispatch code by the restatements in sweep_util.py, which
test_volume_sweep_host.py checks against these very lists):

bf16 fmaps, D >= 33 (two 32-d stages), W2 > 64 -- the LDS-DMA ring kernel
build_bf16_ring_kernel<NWN, FMA, ..>, chosen by csrc/volume.hip,
bf16_ring_shape (fewest padded w2 columns; first of {4,5},{4,4},{3,5},{3,4},
{2,5},{2,4} on ties), launched by launch_bf16_ring / launch_bf16_ring_n:

    plain (2,4)      W2 65-128
    plain (2,5)      W2 129-160
    plain (3,4)      W2 161-192, 321-384
    plain (3,5)      W2 193-240, 385-480, 641-720
    plain (4,4)      W2 241-256, 481-512, 721-768
    plain (4,5)      W2 257-320
    deferred (2,4)   W2 65-128      (bf16 pyramid, levels 0 + 2 stored, 16-B rows)
    deferred (3,4)   W2 129-192
    deferred (4,4)   W2 193-256
    deferred (5,4)   W2 257-320
    records          64 < W2 <= 320, D > 224: deferred (ceil(W2 / 64), 4)
                     (rc_launch_build_bf16mma, RC_LAYOUT_RECORDS)

  nbuf <= 3 runs the 3-level epilogue, nbuf >= 4 the 5-level one
  (kB16MaxFused; launch_bf16_ring_n); levels past the fifth are pooled from
  memory by rc_corr_build (capi.cpp).
bf16 fmaps with W2 <= 64 or D <= 32, and fp32 fmaps with a bf16 pyramid:
  the per-wave kernel build_bf16_kernel<IN_BF16, ALIGNED> (rc_launch_build_bf16mma;
  ALIGNED = W1, W2 multiples of 8 for bf16 fmaps, of 4 for fp32 fmaps).
fp32 fmaps, fp32 pyramid, W1 and W2 multiples of 4: build_split_kernel
  (csrc/volume_split.hip, rc_launch_build_split): rows in ceil(nf / 8) balanced
  tiles of tile_frags(W) 16-column fragments, nf = ceil(W / 16) -- one tile to
  W = 128, two of 5..8 fragments to 256, three to 384, six of 8 + 7 at 720;
  the kernel switches on its tile's (fa, fb) in 1..8 x 1..8.  nbuf <= 3: the
  3-level instance, else the 5-level one (kSpMaxFused); more than two
  workgroups per CU: the three-slot ring (sp_ring3).  With
  RC_LAYOUT_DISPARITY: build_split_kernel<kModeSheared, 3>.
fp32 with RC_BUILD_EXACT_F32, or a width not a multiple of 4
  (rc_launch_build_f32): build_f32_ring_kernel for W1, W2 multiples of 4,
  else build_f32_kernel<false, 2, 0>.
rc_corr_build_backward (csrc/backward.hip, rc_launch_volume_bwd):
  volume_bwd_split_kernel<true, kPairFold | 1 | 2> for W1, W2 multiples of 4
  and pair-folded, 1- or 2-level gradients; otherwise, or with
  RC_BUILD_EXACT_F32, volume_bwd_kernel<vec, NL, 16> (vec = both widths
  multiples of 4).  The width is the reduction dimension of both GEMMs (32-wide
  k steps), D the output dimension (128-row tiles).

Bounds (the project's contracts, SURVEY.md 8d and the modules named):
  fp32 volume: max|d|/max|ref| <= 1e-4 and rel-L2 <= 1e-5 against the fp64
    oracle; the split-bf16 kernel also <= max(2 x the exact kernel's error on
    the same inputs, 1e-6) (test_split_gpu.py);
  bf16 MFMA, fp32 pyramid: <= 1e-5 against the oracle on the bf16 inputs;
    bf16 pyramid: <= 8e-3 (test_corr_gpu.py::test_bf16_mma_vs_oracle);
  pooling: each stored level bit-identical to corr_pool (fp32) / bf16_pool_np
    (bf16) of the level below as stored;
  volume backward: 1e-4 / 1e-5, and split <= 2 x exact + 1e-7 (norm) /
    + 1e-8 (rel-L2) (test_backward_split_gpu.py).
Each test prints the largest error it saw against its bound.
"""
import numpy as np
import pytest
import torch

import sweep_util as su
from golden_util import norm_err, rel_l2, same
from oracle import coracle
from raft_stereo_amd import _lib
from raft_stereo_amd import corr as rcorr
from sweep_util import bf16_pool_np, integer_sweep
from test_corr_gpu import special_coords

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, BF16 = torch.float32, torch.bfloat16
EXACT = _lib.RC_BUILD_EXACT_F32
VOL_TOL, VOL_L2 = 1e-4, 1e-5
B16_F32PYR, B16_BF16PYR = 1e-5, 8e-3


def band_id(b):
    return f"{b[0]}-{b[-1]}"


def fmaps(D, H, W1, W2, seed, dt=F32):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(1, D, H, W1, generator=g).to(dt), torch.randn(1, D, H, W2, generator=g).to(dt)


def oracle_volume(f1, f2):
    B, D, H, W1 = f1.shape
    return coracle.corr_volume(f1.float().numpy(), f2.float().numpy()).reshape(B * H * W1, f2.shape[3])


class Worst:
    """The largest figure seen per name, printed with its bound."""

    def __init__(self, what):
        self.what, self.v = what, {}

    def add(self, name, val, bnd, tag):
        assert val <= bnd, f"{self.what} {tag}: {name} {val:.3e} > {bnd:.3e}"
        if val >= self.v.get(name, (-1.0,))[0]:
            self.v[name] = (val, bnd, tag)

    def report(self):
        for name, (val, bnd, tag) in self.v.items():
            print(f"{self.what}: max {name} {val:.3e} (bound {bnd:.1e}) at {tag}")


# ------------------------------------------------------------ bf16 builds

def check_bf16(form, D, H, W1, W2, phase, worst, in_dt=BF16, pad=None):
    """One bf16-MFMA build in form a (bf16 pyramid, levels 0 + 2 stored), b
    (fp32 pyramid, levels 0 + 2 stored) or c (bf16 pyramid, 7 buffers).  pad
    (form b): rows padded to 16 bytes, else dense (pyr_ld = NULL)."""
    pad = bool(phase & 1) if pad is None else pad
    f1, f2 = fmaps(D, H, W1, W2, 1000 * W1 + 7 * W2 + D, in_dt)
    ref = oracle_volume(f1.bfloat16(), f2.bfloat16())         # what the kernel multiplies
    tag = f"{form} D={D} H={H} W1={W1} W2={W2}"
    if form == "c":
        lv = su.guarded_build(DEV, f1, f2, BF16, 7, pad=True, phase=phase)
        for l in range(1, 7):
            assert same(lv[l], bf16_pool_np(lv[l - 1])), f"{tag}: level {l}"
        worst.add("norm_err bf16 pyramid", norm_err(lv[0], ref), B16_BF16PYR, tag)
        return
    nbuf = min(3, su.max_nbuf(W2, 3))
    stored = (0, 2) if nbuf == 3 else tuple(range(nbuf))
    if form == "a":
        lv = su.guarded_build(DEV, f1, f2, BF16, nbuf, stored, pad=True, phase=phase)
        worst.add("norm_err bf16 pyramid", norm_err(lv[0], ref), B16_BF16PYR, tag)
        pool = bf16_pool_np
    else:
        lv = su.guarded_build(DEV, f1, f2, F32, nbuf, stored, pad=pad, phase=phase)
        worst.add("norm_err fp32 pyramid", norm_err(lv[0], ref), B16_F32PYR, tag)
        pool = coracle.corr_pool
    if nbuf == 3:
        assert same(lv[2], pool(pool(lv[0]))), f"{tag}: level 2"
    elif nbuf == 2:
        assert same(lv[1], pool(lv[0])), f"{tag}: level 1"


@pytest.mark.parametrize("form", ["a", "b", "c"])
@pytest.mark.parametrize("band", su.BF16_W2_BANDS, ids=band_id)
def test_bf16_w2_sweep(band, form):
    worst = Worst(f"bf16 W2 sweep {form}")
    for W2 in band:
        # form b: dense rows at W2 % 4 in (0, 1) -- even and odd row strides
        check_bf16(form, su.BF16_D, 1 + W2 % 2, 24, W2, W2, worst, pad=bool(W2 & 2))
    worst.report()


@pytest.mark.parametrize("W2", [131, 201, 311])
@pytest.mark.parametrize("pyr_dt", [F32, BF16], ids=["f32pyr", "bf16pyr"])
def test_bf16_ring_scalar_rows_regression(W2, pyr_dt):
    """Found by test_bf16_w1_sweep[1-52-311-b] (W1 = 2, W2 = 311, dense fp32
    rows): the plain ring instances with 5 fragments per wave -- (2,5), (3,5),
    (4,5) -- stage an 80-column level-0 image per wave, and a row stride that
    allows only scalar stores (dense rows of an odd width) sent it to
    store_rows16<1> (csrc/epilogue.h) with 80 lanes per row: 64 / 80 = 0 rows
    per instruction, a loop that never advanced (the kernel hung).  Every
    level stored, dense rows."""
    worst = Worst(f"bf16 ring scalar rows W2={W2}")
    for W1, H in ((2, 1), (24, 2)):
        f1, f2 = fmaps(su.BF16_D, H, W1, W2, W1 + W2, BF16)
        ref = oracle_volume(f1, f2)
        lv = su.guarded_build(DEV, f1, f2, pyr_dt, 3, pad=False, phase=W1)
        bf = pyr_dt == BF16
        worst.add("norm_err", norm_err(lv[0], ref), B16_BF16PYR if bf else B16_F32PYR, f"W1={W1} H={H}")
        for l in (1, 2):
            assert same(lv[l], (bf16_pool_np if bf else coracle.corr_pool)(lv[l - 1])), f"level {l}"
    worst.report()


def test_bf16_w2_wide():
    """The second and third ranges of plain (4,4)."""
    worst = Worst("bf16 wide W2")
    for W2 in su.BF16_W2_WIDE:
        check_bf16("b", su.BF16_D, 1, 24, W2, W2 // 8, worst)
    worst.report()


@pytest.mark.parametrize("form", ["a", "b"])
@pytest.mark.parametrize("W2", su.BF16_W1_W2)
@pytest.mark.parametrize("band", su.BF16_W1_BANDS, ids=band_id)
def test_bf16_w1_sweep(band, W2, form):
    worst = Worst(f"bf16 W1 sweep {form} W2={W2}")
    for W1 in band:
        check_bf16(form, su.BF16_D, 1 + W1 % 2, W1, W2, W1, worst)
    worst.report()


@pytest.mark.parametrize("D", su.BF16_DS)
def test_bf16_d_sweep(D):
    worst = Worst(f"bf16 D={D}")
    for i, W2 in enumerate(su.BF16_D_PLAIN_W2):
        check_bf16("b", D, 1 + i % 2, 40, W2, i, worst)
        check_bf16("c", D, 1 + i % 2, 40, W2, i + 1, worst)
    for i, W2 in enumerate(su.BF16_D_DEFER_W2):
        check_bf16("a", D, 2 - i % 2, 40, W2, i, worst)
    worst.report()


def test_bf16_per_wave():
    """bf16 fmaps below the ring's limits: build_bf16_kernel<true, ALIGNED>."""
    worst = Worst("bf16 per-wave")
    for i, (D, W1, W2) in enumerate(su.BF16_PERWAVE):
        for form in ("a", "b"):
            check_bf16(form, D, 1 + i % 2, W1, W2, i, worst)
    worst.report()


@pytest.mark.parametrize("axis", ["W2", "W1"])
def test_f32_fmaps_bf16_pyramid(axis):
    """build_bf16_kernel<false, ..>: fp32 fmaps rounded to bf16 on load."""
    worst = Worst(f"f32 fmaps, bf16 pyramid, {axis} sweep")
    shapes = [(20, w) for w in su.F32IN_W2] if axis == "W2" else [(w, 36) for w in su.F32IN_W1]
    for W1, W2 in shapes:
        check_bf16("a", su.F32IN_D, 1 + (W1 + W2) % 2, W1, W2, W1 + W2, worst, in_dt=F32)
    worst.report()


# ---------------------------------------------------------------- records

def record_padding_zero(rec, W2):
    """Slots whose element lies outside its level's width hold zeros
    (include/raftcorr.h, RC_LAYOUT_RECORDS)."""
    P, NR, S = rec.shape
    r = np.arange(NR)[:, None]
    s = np.arange(S)[None, :]
    e2, e0 = 4 * r - 14 + s, 16 * r - 26 + (s - 26)
    outside = np.where(s < 26, (e2 < 0) | (e2 >= W2 >> 2), (e0 < 0) | (e0 >= W2))
    bits = rec.contiguous().view(torch.int16).cpu().numpy()
    return not (bits[:, outside] & 0x7FFF).any()


@pytest.mark.parametrize("band", su.REC_W2_BANDS, ids=band_id)
def test_records_vs_rows_and_oracle(band):
    """RC_LAYOUT_RECORDS: levels 0 and 2 gathered from the records equal the
    row layout's stored levels bit for bit, the padding slots are zero, and
    the record lookup equals the oracle's lookup on those levels directly."""
    worst = Worst("records")
    for W2 in band:
        for W1 in su.REC_W1:
            for D in su.REC_D:
                tag = f"D={D} W1={W1} W2={W2}"
                f1, f2 = fmaps(D, 1, W1, W2, 31 * W2 + W1 + D, BF16)
                rows = su.guarded_build(DEV, f1, f2, BF16, 3, (0, 2), pad=True, phase=W2)
                worst.add("norm_err bf16 pyramid", norm_err(rows[0], oracle_volume(f1, f2)), B16_BF16PYR, tag)
                ar, rec = su.guarded_records(DEV, f1, f2, phase=W2 + W1)
                assert record_padding_zero(rec, W2), f"{tag}: padding slot not zero"
                lv = {}
                for l in (0, 2):
                    lv[l] = rcorr.records_level(rec, l, W2).reshape(W1, -1).float().cpu().numpy()
                    assert same(lv[l], rows[l]), f"{tag}: level {l} records != rows"
                pyr = [lv[0], bf16_pool_np(lv[0]), lv[2], bf16_pool_np(lv[2])]
                g = torch.Generator().manual_seed(W2 + D)
                xs = special_coords(1, 1, 70, W2, g)[0, 0, 0].numpy()
                if W1 == 70:
                    xs = np.concatenate([xs, integer_sweep(W2)])
                xs = np.concatenate([xs, np.zeros(-len(xs) % W1, np.float32)])
                for x in xs.reshape(-1, W1):
                    c = np.zeros((1, 2, 1, W1), np.float32)
                    c[0, 0, 0] = x
                    got = rcorr.lookup_records(rec, torch.from_numpy(c).to(DEV), 4, W2).cpu().numpy()
                    assert same(got, coracle.corr_lookup(pyr, c, 4, 4)), f"{tag}: lookup"
                ar.assert_guards_intact()              # the lookups wrote nothing into the arena
    worst.report()


# ------------------------------------------------------------ fp32 builds

def check_split(D, H, W1, W2, phase, worst):
    """Split-bf16 build, lazy (3-level instance) and eager (5-level
    instance), against the oracle and the exact fp32 kernel."""
    f1, f2 = fmaps(D, H, W1, W2, 77 * W1 + 3 * W2 + D)
    ref = oracle_volume(f1, f2)
    tag = f"D={D} H={H} W1={W1} W2={W2}"
    ex = su.guarded_build(DEV, f1, f2, F32, 1, flags=EXACT, phase=phase)[0]
    lazy = su.guarded_build(DEV, f1, f2, F32, 3, (0, 2), pad=bool(phase & 1), phase=phase)
    ne = su.max_nbuf(W2, 5)
    eager = su.guarded_build(DEV, f1, f2, F32, ne, pad=not phase & 1, phase=phase + 1)
    e_ex, l_ex = norm_err(ex, ref), rel_l2(ex, ref)
    worst.add("exact norm_err", e_ex, VOL_TOL, tag)
    worst.add("exact rel_l2", l_ex, VOL_L2, tag)
    e, l2 = norm_err(lazy[0], ref), rel_l2(lazy[0], ref)
    worst.add("split norm_err", e, VOL_TOL, tag)
    worst.add("split rel_l2", l2, VOL_L2, tag)
    worst.add("split norm_err / max(2 exact, 1e-6)", e / max(2 * e_ex, 1e-6), 1.0, tag)
    worst.add("split rel_l2 / max(2 exact, 1e-6)", l2 / max(2 * l_ex, 1e-6), 1.0, tag)
    assert same(eager[0], lazy[0]), f"{tag}: eager level 0 != lazy"
    assert same(lazy[2], coracle.corr_pool(coracle.corr_pool(lazy[0]))), f"{tag}: lazy level 2"
    for l in range(1, ne):
        assert same(eager[l], coracle.corr_pool(eager[l - 1])), f"{tag}: eager level {l}"


@pytest.mark.parametrize("band", su.SPLIT_CROSS_BANDS, ids=band_id)
def test_split_fragment_pairs(band):
    worst = Worst("split fragment pairs")
    for W1 in band:
        for W2 in su.M4:
            check_split(su.F32_D, 1, W1, W2, (W1 + W2) // 4, worst)
    worst.report()


@pytest.mark.parametrize("shapes", su.bands(su.BAL_SHAPES, 34), ids=lambda b: f"{b[0][0]}x{b[0][1]}")
def test_split_balanced_tiles(shapes):
    worst = Worst("split balanced tiles")
    for W1, W2 in shapes:
        check_split(su.F32_D, 1, W1, W2, (W1 + W2) // 4, worst)
    worst.report()


@pytest.mark.parametrize("D", su.SPLIT_DS)
def test_split_d_states(D):
    worst = Worst(f"split D={D}")
    for i, (W1, W2) in enumerate(su.SPLIT_D_SHAPES):
        check_split(D, 1, W1, W2, i, worst)
    worst.report()


@pytest.mark.parametrize("D", su.RING3_DS)
def test_split_ring3_d_states(D):
    """More than two workgroups per CU: the three-slot ring (sp_ring3)."""
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    worst = Worst(f"split three-slot ring D={D}")
    check_split(D, 2 * ncu + 2, 16, 16, D, worst)
    worst.report()


def check_exact(D, H, W1, W2, nbuf, phase, worst):
    f1, f2 = fmaps(D, H, W1, W2, 13 * W1 + 5 * W2 + nbuf)
    ref = oracle_volume(f1, f2)
    tag = f"D={D} W1={W1} W2={W2} nbuf={nbuf}"
    lv = su.guarded_build(DEV, f1, f2, F32, nbuf, pad=bool(phase & 1), flags=EXACT, phase=phase)
    worst.add("exact norm_err", norm_err(lv[0], ref), VOL_TOL, tag)
    worst.add("exact rel_l2", rel_l2(lv[0], ref), VOL_L2, tag)
    for l in range(1, nbuf):
        assert same(lv[l], coracle.corr_pool(lv[l - 1])), f"{tag}: level {l}"


@pytest.mark.parametrize("axis", ["W2", "W1"])
def test_exact_f32_any_width(axis):
    """build_f32_kernel<false, 2, 0>: widths not multiples of 4."""
    worst = Worst(f"exact fp32 any width, {axis} sweep")
    shapes = [(21, w) for w in su.EXACT_W2] if axis == "W2" else [(w, 37) for w in su.EXACT_W1]
    for W1, W2 in shapes:
        for nbuf in sorted({1, su.max_nbuf(W2, 5)}):
            check_exact(su.F32_D, 1, W1, W2, nbuf, W1 + W2 + nbuf, worst)
    worst.report()


@pytest.mark.parametrize("shapes", su.bands(su.EXACT_VEC_SHAPES, 72), ids=lambda b: f"{b[0][0]}x{b[0][1]}")
def test_exact_f32_vector_ring(shapes):
    """build_f32_ring_kernel: W1, W2 multiples of 4 with RC_BUILD_EXACT_F32."""
    worst = Worst("exact fp32 vector ring")
    for W1, W2 in shapes:
        check_exact(su.F32_D, 1, W1, W2, su.max_nbuf(W2, 5), (W1 + W2) // 4, worst)
    worst.report()


@pytest.mark.parametrize("shapes", su.bands(su.DISP_SHAPES, 66), ids=lambda b: f"{b[0][0]}x{b[0][1]}")
def test_disparity_layout(shapes):
    """RC_LAYOUT_DISPARITY: levels 0 and 2 unsheared equal the row layout's."""
    for W1, W2 in shapes:
        f1, f2 = fmaps(su.F32_D, 1, W1, W2, 5 * W1 + W2)
        phase = (W1 + W2) // 4
        rows = su.guarded_build(DEV, f1, f2, F32, 3, (0, 2), pad=True, phase=phase)
        ar, S = su.guarded_sheared(DEV, f1, f2, 4, phase=phase + 1)
        for l in (0, 2):
            got = rcorr.unshear_level(S[l], l, 1, 1, W1, W2).reshape(W1, -1).cpu().numpy()
            assert np.isfinite(got).all(), (W1, W2, l)
            assert same(got, rows[l]), f"W1={W1} W2={W2}: level {l}"


# -------------------------------------------------------- volume backward

def make_grads(P, W2, nlev, present, g):
    """Random level gradients: the kernel's buffers (rows padded to 4 floats
    with zeros, None for a folded level) and the oracle's per-level list."""
    bufs, per = [], []
    for l in range(nlev):
        W = W2 >> l
        if l not in present:
            bufs.append(None)
            per.append(np.zeros((P, W), np.float32))
            continue
        v = torch.randn(P, W, generator=g)
        b = torch.zeros(P, su.grad_ld(W))
        b[:, :W] = v
        bufs.append(b)
        per.append(v.numpy())
    return bufs, per


LAYOUTS = {"pair4": (3, (0, 2)), "pair2": (1, (0,)), "level2": (2, (0, 1)),
           "level1": (1, (0,)), "level3": (3, (0, 1, 2))}


def check_bwd(D, H, W1, W2, layout, phase, worst, split):
    """split: the default path is the split-bf16 kernel (compare it with the
    exact one too); else only the exact kernel runs for this shape."""
    g = torch.Generator().manual_seed(D + 11 * W1 + 101 * W2)
    f1 = torch.randn(1, D, H, W1, generator=g)
    f2 = torch.randn(1, D, H, W2, generator=g)
    nlev, present = LAYOUTS[layout]
    bufs, per = make_grads(H * W1, W2, nlev, present, g)
    refs = coracle.corr_build_backward(f1.numpy(), f2.numpy(), per)
    tag = f"{layout} D={D} H={H} W1={W1} W2={W2}"
    ex = su.guarded_build_backward(DEV, f1, f2, bufs, exact=True, phase=phase)
    got = su.guarded_build_backward(DEV, f1, f2, bufs, exact=False, phase=phase + 1) if split else ex
    for name, a, e, ref in (("dF1", got[0], ex[0], refs[0]), ("dF2", got[1], ex[1], refs[1])):
        ee, le = norm_err(e, ref), rel_l2(e, ref)
        worst.add(f"exact {name} norm_err", ee, VOL_TOL, tag)
        worst.add(f"exact {name} rel_l2", le, VOL_L2, tag)
        if split:
            es, ls = norm_err(a, ref), rel_l2(a, ref)
            worst.add(f"split {name} norm_err", es, VOL_TOL, tag)
            worst.add(f"split {name} rel_l2", ls, VOL_L2, tag)
            worst.add(f"split {name} norm_err / (2 exact + 1e-7)", es / (2 * ee + 1e-7), 1.0, tag)
            worst.add(f"split {name} rel_l2 / (2 exact + 1e-8)", ls / (2 * le + 1e-8), 1.0, tag)


@pytest.mark.parametrize("layout", su.BWD_LAYOUTS)
@pytest.mark.parametrize("shapes", su.bands(su.BWD_SHAPES, 80), ids=lambda b: f"{b[0][0]}x{b[0][1]}")
def test_backward_split_widths(shapes, layout):
    worst = Worst(f"backward split {layout}")
    for W1, W2 in shapes:
        if su.bwd_layout_ok(layout, W2):
            check_bwd(su.BWD_D, 1 + (W1 // 4) % 2, W1, W2, layout, (W1 + W2) // 4, worst, True)
    worst.report()


@pytest.mark.parametrize("layout", ["level1", "level2", "level3", "pair4"])
@pytest.mark.parametrize("axis", ["W2", "W1"])
def test_backward_exact_widths(axis, layout):
    """volume_bwd_kernel<false, ..>: widths not multiples of 4."""
    worst = Worst(f"backward exact {layout}, {axis} sweep")
    shapes = [(21, w) for w in su.BWD_EXACT_W2] if axis == "W2" else [(w, 37) for w in su.BWD_EXACT_W1]
    # capi.cpp, rc_corr_build_backward: `(W2 >> (levels - 1)) < 1` is RC_EINVAL
    need = {"level1": 1, "level2": 2, "level3": 4, "pair4": 4}[layout]
    for W1, W2 in shapes:
        if W2 >= need:
            check_bwd(su.BWD_D, 1 + (W1 + W2) % 2, W1, W2, layout, W1 + W2, worst, False)
    worst.report()


@pytest.mark.parametrize("D", su.BWD_DS)
def test_backward_d_sweep(D):
    worst = Worst(f"backward D={D}")
    for i, (W1, W2) in enumerate(su.BWD_D_SHAPES):
        check_bwd(D, 1, W1, W2, "pair4", i, worst, W1 % 4 == 0 and W2 % 4 == 0)
    worst.report()
