"""CorrBlock1D(pyramid_dtype=torch.float16) on the GPU: the
fp16 MFMA build (ring and per-wave kernels, fp16 and fp32 fmaps), the fp16
pooling, the per-level and pair lookups over fp16 levels, overflow, autograd,
the refusals, and the network option.

References: the fp64-accumulated C oracle (``coracle.corr_pyramid``) on the
fp16-rounded fmaps for level values; numpy for the pooling -- level i is
``((a + b) * 0.5).astype(np.float16)`` of stored level i - 1, in fp32; the C
oracle's lookup (``coracle.corr_lookup``) on the stored levels for the lookup
output.  Everything but the level values against the fp64 oracle is compared
bit for bit (NaN == NaN)."""
import functools

import numpy as np
import pytest
import torch

from golden_util import norm_err, same
from oracle import coracle
from raft_stereo_amd import CorrBlock1D
from raft_stereo_amd import corr as rcorr

from sweep_util import f16_pool_np
from test_corr_gpu import pyr_np, special_coords
from test_out_dtype_gpu import assert_same_half

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F16 = torch.float16

# One fp16 rounding of each stored value: the bf16 pyramid's 8e-3
# (test_corr_gpu.test_bf16_mma_vs_oracle) scaled by the 2^-3 ratio of the two
# formats' rounding units.
F16_TOL = 1e-3


# ------------------------------------------------------------ 1. pyramid vs oracle
# test_corr_gpu.BF16_SHAPES: the ring kernel (2 / 3 waves along w2, 4 / 5
# fragments), the per-wave kernel (W2 <= 64, or fp32 fmaps), rows that are not
# 16-B aligned, D % 32 != 0, idle waves, 3 levels (the per-level lookup)
F16_SHAPES = [
    (1, 256, 2, 64, 64, 4, 4),
    (2, 256, 2, 311, 311, 4, 4),
    (1, 96, 3, 40, 57, 3, 3),
    (1, 37, 2, 24, 33, 4, 2),
    (1, 64, 2, 700, 720, 4, 4),
    (1, 256, 1, 150, 130, 3, 4),
    (1, 40, 2, 100, 100, 4, 2),
]


@functools.lru_cache(maxsize=None)
def _case(shape):
    """fmaps, coords and the oracle pyramid of the fp16-rounded fmaps: computed
    once per shape, shared by both modes, never modified."""
    B, D, H, W1, W2, L, r = shape
    g = torch.Generator().manual_seed(7 + sum(shape))
    f1 = torch.randn(B, D, H, W1, generator=g)
    f2 = torch.randn(B, D, H, W2, generator=g)
    x = torch.arange(W1).float().view(1, 1, 1, W1) - torch.rand(B, 1, H, W1, generator=g) * 40
    coords = torch.cat([x, torch.zeros_like(x)], 1)
    ref = coracle.corr_pyramid(f1.half().float().numpy(), f2.half().float().numpy(), L)
    return f1, f2, coords, ref


@pytest.mark.parametrize("shape", F16_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("mode", ["f16in_f16pyr", "f32in_f16pyr"])
def test_f16_mma_vs_oracle(shape, mode):
    B, D, H, W1, W2, L, r = shape
    f1, f2, coords, ref = _case(shape)
    in_dt = torch.float32 if mode.startswith("f32in") else F16
    with torch.no_grad():
        blk = CorrBlock1D(f1.to(DEV, in_dt), f2.to(DEV, in_dt), num_levels=L, radius=r, pyramid_dtype=F16)
        out = blk(coords.to(DEV)).cpu().numpy()
    assert blk.pyramid_dtype == F16 and all(t.dtype == F16 for t in blk.corr_pyramid)
    got = pyr_np(blk)
    for i in range(L + 1):
        err = norm_err(got[i], ref[i])
        print(f"{mode} {shape} level {i}: normalised error {err:.3e}")
        assert err <= F16_TOL, f"level {i}: {err}"
    for i in range(1, L + 1):
        assert same(got[i], f16_pool_np(got[i - 1])), f"level {i} != fp16 pool of stored level {i - 1}"
    # the lookup reads the stored fp16 levels exactly
    assert out.dtype == np.float32
    assert same(out, coracle.corr_lookup(got[:L], coords.numpy(), L, r))


# ------------------------------------------------------------------ 2. pair lookup
# test_corr_gpu.BF16_PAIR_SHAPES
F16_PAIR_SHAPES = [
    (2, 64, 3, 240, 240, 4, 4),
    (1, 32, 2, 311, 311, 4, 4),     # config-3 width: odd level widths
    (1, 16, 3, 45, 45, 4, 3),
    (1, 16, 2, 50, 50, 2, 4),
    (1, 8, 2, 20, 16, 4, 1),
]


@pytest.mark.parametrize("shape", F16_PAIR_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("fmap_dt", [F16, torch.float32], ids=["f16in", "f32in"])
def test_f16_pair_lookup_bitexact(shape, fmap_dt):
    """The lazy block (levels 0 and 2 stored, 1 and 3 derived and rounded to
    fp16 in registers) equals the eager block with every level materialised
    and the per-level lookup over that pyramid, bit for bit, NaN / inf /
    subnormal coords included: with and without shadow copies, NCHW and
    channels-last, and with an fp16 / bf16 output equal to ``.to(dtype)`` of
    the fp32 output."""
    B, D, H, W1, W2, L, r = shape
    g = torch.Generator().manual_seed(700 + sum(shape))
    f1 = torch.randn(B, D, H, W1, generator=g).to(DEV, fmap_dt)
    f2 = torch.randn(B, D, H, W2, generator=g).to(DEV, fmap_dt)
    coords = special_coords(B, H, W1, W2, g).to(DEV)
    with torch.no_grad():
        eager = CorrBlock1D(f1, f2, num_levels=L, radius=r, pyramid_dtype=F16, lazy_levels=False)
        assert eager.levels_stored == list(range(L + 1))
        c = eager(coords)
        le = pyr_np(eager)
        b = rcorr.lookup(eager.corr_pyramid, coords, L, r)          # the per-level kernel
        assert same(c.cpu().numpy(), b.cpu().numpy())
        for shadow in (False, True):
            for cl in (False, True):
                what = f"shadow={shadow} channels_last={cl}"
                blk = CorrBlock1D(f1, f2, num_levels=L, radius=r, pyramid_dtype=F16, shadow=shadow,
                                  channels_last=cl)
                assert blk._chain and blk.levels_stored == ([0, 2] if L == 4 else [0])
                assert blk._shadow == (frozenset(blk.levels_stored) if shadow else frozenset())
                a = blk(coords)
                assert a.dtype == torch.float32
                assert a.is_contiguous(memory_format=torch.channels_last if cl else torch.contiguous_format)
                assert same(a.cpu().numpy(), c.cpu().numpy()), what
                for od in (torch.float16, torch.bfloat16):
                    blk.out_dtype = od                               # read at call time
                    assert_same_half(blk(coords), a, od, f"{what} out_dtype={od}")
                blk.out_dtype = None
        lv = pyr_np(blk)
    for i in range(L + 1):
        assert same(lv[i], le[i]), f"lazy vs fused epilogue, level {i}"
        if i:
            assert same(lv[i], f16_pool_np(lv[i - 1])), f"level {i} != fp16 pool of level {i - 1}"


# --------------------------------------------------------------------- 3. overflow
@pytest.mark.parametrize("fmap_dt", [F16, torch.float32], ids=["f16in", "f32in"])
def test_f16_overflow_stores_inf(fmap_dt):
    """D = 32, fmap1 = 512, fmap2 = +-512: every volume entry is
    +-32 * 2^18 / sqrt(32) = +-1.48e6, above fp16's 65504, and is stored as
    +-inf with fmap2's sign (what ``.half()`` gives); a level above is the
    fp16 pool of the level below as stored, so +inf and -inf pool to NaN."""
    B, D, H, W1, W2, L = 1, 32, 2, 40, 72, 4
    sign = torch.ones(H, W2)
    sign[0, 1::3] = -1.0                                   # fixed pattern: pairs of equal and of opposite sign
    sign[1, 2::5] = -1.0
    sign[1, 40:] = -1.0
    f1 = torch.full((B, D, H, W1), 512.0)
    f2 = (512.0 * sign).view(1, 1, H, W2).expand(B, D, H, W2).contiguous()
    want0 = (sign * float("inf")).view(H, 1, W2).expand(H, W1, W2).reshape(H * W1, W2).numpy()
    with torch.no_grad():
        for lazy in (None, False):                         # pooled by rc_corr_pool / by the fused epilogue
            blk = CorrBlock1D(f1.to(DEV, fmap_dt), f2.to(DEV, fmap_dt), num_levels=L, radius=4,
                              pyramid_dtype=F16, lazy_levels=lazy)
            got = pyr_np(blk)
            assert same(got[0], want0), f"lazy_levels={lazy}"
            assert np.isnan(f16_pool_np(got[0])).any()     # the pattern does pool +inf with -inf
            for i in range(1, L + 1):
                assert same(got[i], f16_pool_np(got[i - 1])), f"lazy_levels={lazy}: level {i}"


# -------------------------------------------------------------------- 4. gradients
def test_f16_pyramid_gradients():
    """fp16 fmaps with requires_grad: the gradients come back as fp16 and are
    ``.half()`` of those of an fp32-pyramid block on the same fmaps widened
    to fp32 -- the lookup backward does not read the pyramid and the build
    backward runs on the widened fmaps: same kernels, same inputs."""
    B, D, H, W, L, r = 1, 32, 2, 64, 4, 4
    g = torch.Generator().manual_seed(41)
    h1 = torch.randn(B, D, H, W, generator=g).half()
    h2 = torch.randn(B, D, H, W, generator=g).half()
    x = torch.arange(W).float().view(1, 1, 1, W) - torch.rand(B, 1, H, W, generator=g) * 20
    coords = torch.cat([x, torch.zeros_like(x)], 1).to(DEV)
    wgt = torch.randn(B, L * (2 * r + 1), H, W, generator=g).to(DEV)

    def grads(f1, f2, **kw):
        f1 = f1.to(DEV).requires_grad_()
        f2 = f2.to(DEV).requires_grad_()
        blk = CorrBlock1D(f1, f2, num_levels=L, radius=r, **kw)
        out = blk(coords)
        assert out.dtype == torch.float32
        (out * wgt).sum().backward()
        return f1.grad, f2.grad

    a1, a2 = grads(h1, h2, pyramid_dtype=F16)
    b1, b2 = grads(h1.float(), h2.float())
    assert a1.dtype == a2.dtype == F16 and b1.dtype == torch.float32
    assert float(b1.abs().max()) > 0 and float(b2.abs().max()) > 0
    assert torch.equal(a1, b1.half()) and torch.equal(a2, b2.half())


# -------------------------------------------------------------------- 5. refusals
def test_f16_pyramid_refusals():
    """What has no fp16-pyramid kernel raises, naming the option; nothing is
    answered from a bf16 pyramid."""
    f = torch.randn(1, 256, 2, 128, device=DEV).half()
    coords = rcorr.coords_grid(1, 2, 128, device=DEV)
    w = torch.randn(8, 36, 1, 1, device=DEV)
    with torch.no_grad():
        blk = CorrBlock1D(f, f, num_levels=4, radius=4, pyramid_dtype=F16)
        assert blk.pyramid_dtype == F16 and blk.layout == "rows"
        with pytest.raises(RuntimeError, match="lookup_step.*float16"):
            blk.lookup_step(coords)
        for diff in (False, True):
            with pytest.raises(RuntimeError, match="lookup_convc1.*float16"):
                blk.lookup_convc1(coords, w, differentiable=diff)
        for layout in ("records", "disparity"):
            with pytest.raises(ValueError, match=layout):
                CorrBlock1D(f, f, num_levels=4, radius=4, pyramid_dtype=F16, layout=layout)
        assert CorrBlock1D(f, f, num_levels=4, radius=4, pyramid_dtype=F16, layout="auto").layout == "rows"
        with pytest.raises(ValueError, match="bfloat16"):
            CorrBlock1D(f.bfloat16(), f.bfloat16(), pyramid_dtype=F16)
        # unchanged: fp16 fmaps without the option still give a bf16 pyramid
        assert CorrBlock1D(f, f).pyramid_dtype == torch.bfloat16
        # 3 levels and low_latency go to the per-level lookup
        assert not CorrBlock1D(f, f, num_levels=3, pyramid_dtype=F16)._chain
        assert not CorrBlock1D(f, f, num_levels=4, pyramid_dtype=F16, low_latency=True)._chain


# --------------------------------------------------------------------- 6. network
def test_network_corr_pyramid_dtype_autocast():
    """RAFTStereo(corr_pyramid_dtype="autocast") under fp16 autocast: the corr
    block receives the encoders' fp16 fmaps and pyramid_dtype=torch.float16
    (without the option: the same fmaps and no keyword, i.e. the bf16
    pyramid); the predictions are finite and no further from the same network
    on an fp32 pyramid (fmaps widened) than the bf16 default's are."""
    from raft_stereo_amd.network import RAFTStereo, StereoArgs

    g = torch.Generator().manual_seed(8)
    img1 = (torch.rand(1, 3, 64, 96, generator=g) * 255).to(DEV)
    img2 = torch.roll(img1, -4, dims=-1)
    args = StereoArgs(mixed_precision=True)
    seen = []

    class Spy(CorrBlock1D):
        widen = False

        def __init__(self, fmap1, fmap2, **kw):
            seen.append((fmap1.dtype, fmap2.dtype, kw.get("pyramid_dtype", "unset")))
            if self.widen:                                   # the fp32-pyramid reference
                fmap1, fmap2 = fmap1.float(), fmap2.float()
            super().__init__(fmap1, fmap2, **kw)
            seen.append(self.pyramid_dtype)

    class SpyF32(Spy):
        widen = True

    def run(block, **kw):
        torch.manual_seed(0)
        model = RAFTStereo(args, corr_block=block, **kw).eval().to(DEV)
        del seen[:]
        with torch.no_grad():
            preds = model(img1, img2, iters=3)
        assert len(preds) == 3
        return torch.cat([p.float().cpu().reshape(-1) for p in preds]), list(seen)

    def measure():
        ref, s = run(SpyF32)
        assert s == [(F16, F16, "unset"), torch.float32]
        new, s = run(Spy, corr_pyramid_dtype="autocast")
        assert s == [(F16, F16, F16), F16], s
        old, s = run(Spy)
        assert s == [(F16, F16, "unset"), torch.bfloat16], s    # nothing changes without the option
        assert bool(torch.isfinite(new).all()) and bool(torch.isfinite(old).all())
        d_new, d_old = (new - ref).abs().mean().item(), (old - ref).abs().mean().item()
        print(f"MAE vs the fp32-pyramid network: fp16 pyramid {d_new:.3e} px, bf16 default {d_old:.3e} px")
        return d_new, d_old

    # the GPU library's half-precision convolutions are not bit-reproducible on
    # every run (test_out_dtype_gpu.py): deterministic algorithms are asked
    # for, and everything is run once more before the path is blamed
    det = (torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark)
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    try:
        d_new, d_old = measure()
        if d_new > d_old:
            d_new, d_old = measure()
    finally:
        torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = det
    assert d_new <= d_old, (d_new, d_old)
