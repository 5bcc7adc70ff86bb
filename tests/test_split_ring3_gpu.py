"""The three-slot LDS-DMA ring of the split-bf16 fp32 volume
(csrc/volume_split.hip, SpRing<128, 3>: three workgroups per CU), its 3-level
and its 5-level instance, against the C oracle's fp64 volume, the exact fp32
MFMA kernel and the four-slot kernel.

Which ring a build runs is the product's choice (sp_ring3: three slots on
grids of more than two workgroups per CU), so:
  * test_ring3_vs_oracle_and_pooling runs the issue's B = 2, H = 3 shapes
    through the product: on these small grids that is the FOUR-slot kernel
    (the shapes' unchanged path);
  * test_ring3_product_grid repeats every D state, with every width class
    among them, on grids just over two workgroups per CU of the device the
    test runs on: the product's THREE-slot kernels against the oracle, lazy
    (3-level instance) and eager (5-level instance);
  * test_ring3_bit_identical_to_four_slots (dev library only) forces three
    (103) and four (104) slots on every B = 2, H = 3 shape, both instances,
    and compares them bit for bit.

Bounds are tests/test_split_gpu.py's: level 0 within the fp32 contract
(max|d|/max|ref| <= 1e-4, rel-L2 <= 1e-5) and at most twice the exact fp32
kernel's own error (or 1e-6); every stored level bit-exact from pooling
(avg_pool2d's fp32 ops) of the level below.

D picks the ring state (a stage is 16 d, a K step two stages, three slots):
16 one half-filled K step; 32 one K step, prologue only; 40 rows d >= D inside
a stage; 64 the first mid-step refill; 96 the first slot reused in its second
role; 128 every slot reused in both roles; 256 the workload's.
(W1, W2) picks the waves' shares: (16, 16) three waves without columns;
(128, 128) full tiles; (240, 240) tiles of 8 + 7 fragments; (160, 160) tiles
of 5; (132, 72) unequal tiles and column tails.
"""
import os

import pytest
import torch

from golden_util import norm_err, rel_l2, same
from oracle import coracle
from raft_stereo_amd import CorrBlock1D
from raft_stereo_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, H = 2, 3

WIDTHS = [(16, 16), (128, 128), (240, 240), (160, 160), (132, 72)]
SHAPES = [(D, w1, w2) for D in (16, 32, 40, 64, 96, 128) for (w1, w2) in WIDTHS] + [(256, 240, 240)]


def fmaps(D, W1, W2):
    g = torch.Generator().manual_seed(7 * D + W1 + 3 * W2)
    return torch.randn(B, D, H, W1, generator=g), torch.randn(B, D, H, W2, generator=g)


def flat(t):
    return t.reshape(t.shape[0], -1).cpu().numpy()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_ring3_vs_oracle_and_pooling(shape):
    D, W1, W2 = shape
    f1, f2 = fmaps(D, W1, W2)
    ref = coracle.corr_volume(f1.numpy(), f2.numpy()).reshape(B * H * W1, W2)
    with torch.no_grad():
        ex = CorrBlock1D.corr(f1.to(DEV), f2.to(DEV), exact_f32=True).reshape(-1, W2).cpu().numpy()
        # the product default: levels 0 and 2 written by the build (the
        # 3-level instance), the others pooled from them
        lazy = CorrBlock1D(f1.to(DEV), f2.to(DEV))
        stored = list(lazy.levels_stored)
        pl = [flat(t) for t in lazy.corr_pyramid]
        # every level written by the build's epilogue (the 5-level instance)
        eager = CorrBlock1D(f1.to(DEV), f2.to(DEV), lazy_levels=False)
        pe = [flat(t) for t in eager.corr_pyramid]
    e_sp, e_ex = norm_err(pl[0], ref), norm_err(ex, ref)
    l_sp, l_ex = rel_l2(pl[0], ref), rel_l2(ex, ref)
    print(f"{shape}: split {e_sp:.2e}/{l_sp:.2e}  exact-f32 {e_ex:.2e}/{l_ex:.2e}  stored {stored}")
    assert e_sp <= 1e-4 and l_sp <= 1e-5
    assert e_sp <= max(2 * e_ex, 1e-6) and l_sp <= max(2 * l_ex, 1e-6)
    assert 0 in stored and len(stored) >= 2
    for p in (pl, pe):
        for l in range(1, len(p)):
            assert same(p[l], coracle.corr_pool(p[l - 1])), f"level {l}"
    assert same(pe[0], pl[0])


# The product runs the three-slot ring on grids of more than two workgroups
# per CU (volume_split.hip, sp_ring3): every D state and every width class
# once more, B = 1 and H just large enough for that on the device at hand
# (256 CUs: 514 rows of one tile, 130 rows of four).  (D, W1, W2, tiles per row)
BIG = [(16, 16, 16, 1), (32, 128, 128, 1), (40, 16, 16, 1), (64, 160, 160, 4), (96, 132, 72, 2),
       (128, 240, 240, 4), (256, 240, 240, 4)]


@pytest.mark.parametrize("shape", BIG, ids=lambda s: "x".join(map(str, s[:3])))
def test_ring3_product_grid(shape):
    D, W1, W2, tiles = shape
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    Hb = 2 * ncu // tiles + 2                      # tiles * Hb > 2 * ncu workgroups
    assert tiles * Hb > 2 * ncu
    g = torch.Generator().manual_seed(D + W1)
    f1 = torch.randn(1, D, Hb, W1, generator=g)
    f2 = torch.randn(1, D, Hb, W2, generator=g)
    ref = coracle.corr_volume(f1.numpy(), f2.numpy()).reshape(Hb * W1, W2)
    with torch.no_grad():
        ex = CorrBlock1D.corr(f1.to(DEV), f2.to(DEV), exact_f32=True).reshape(-1, W2).cpu().numpy()
        # lazy: the 3-level instance; eager: the 5-level instance
        pl = [flat(t) for t in CorrBlock1D(f1.to(DEV), f2.to(DEV)).corr_pyramid]
        pe = [flat(t) for t in CorrBlock1D(f1.to(DEV), f2.to(DEV), lazy_levels=False).corr_pyramid]
    e_ex, l_ex = norm_err(ex, ref), rel_l2(ex, ref)
    for name, p in (("lazy", pl), ("eager", pe)):
        e_sp, l_sp = norm_err(p[0], ref), rel_l2(p[0], ref)
        print(f"{shape} H={Hb} {name}: split {e_sp:.2e}/{l_sp:.2e}  exact-f32 {e_ex:.2e}/{l_ex:.2e}")
        assert e_sp <= 1e-4 and l_sp <= 1e-5, name
        assert e_sp <= max(2 * e_ex, 1e-6) and l_sp <= max(2 * l_ex, 1e-6), name
        for l in range(1, len(p)):
            assert same(p[l], coracle.corr_pool(p[l - 1])), f"{name} level {l}"
    assert same(pe[0], pl[0])


if os.path.exists(_lib.DEV_LIB_PATH):
    # only where the dev library (the A/B build with the four-slot kernel
    # behind RAFTCORR_SPLIT_RING) is present: not defined otherwise

    @pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
    def test_ring3_bit_identical_to_four_slots(shape, monkeypatch):
        """Levels 0 and 2 of the lazy build (3-level instance) and every level
        of the eager build (5-level instance): the product (whichever ring its
        dispatch picks) and the three-slot kernels forced on the shape (103)
        equal the four-slot kernels' (104)."""
        D, W1, W2 = shape
        f1, f2 = fmaps(D, W1, W2)
        f1, f2 = f1.to(DEV), f2.to(DEV)

        def levels():
            blk = CorrBlock1D(f1, f2)
            eager = CorrBlock1D(f1, f2, lazy_levels=False)
            return ([blk.corr_pyramid[0].clone(), blk.corr_pyramid[2].clone()] +
                    [t.clone() for t in eager.corr_pyramid])

        with torch.no_grad():
            prod = levels()
            out = {}
            with _lib.dev_library():
                for ring in ("103", "104"):
                    monkeypatch.setenv("RAFTCORR_SPLIT_RING", ring)
                    out[ring] = levels()
                monkeypatch.delenv("RAFTCORR_SPLIT_RING")
        assert len(out["104"]) == 7
        for name, got in (("three slots", out["103"]), ("product", prod)):
            for l, (x, y) in enumerate(zip(got, out["104"])):
                assert torch.equal(x.view(torch.int32), y.view(torch.int32)), (name, l)
