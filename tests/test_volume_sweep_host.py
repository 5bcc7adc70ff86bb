"""Host-side companion of test_volume_sweep_gpu.py (no GPU): the sweep lists
cover every tile geometry of the dispatch rules as sweep_util.py restates
them, the bounds the sweeps use notice a single wrong element of the oracle's
own output, and the guarded arena keeps its books."""
import numpy as np
import pytest
import torch

import sweep_util as su
from golden_util import norm_err, rel_l2
from oracle import coracle

TAILS16 = {0, 4, 8, 12}


# ---------------------------------------------------------------- coverage

def test_tile_frags_restatement():
    """csrc/volume_split.hip, rc_launch_build_split: the examples its comment
    gives (W = 160: two tiles of 5; W = 240: 8 + 7) and the tile counts."""
    assert su.split_tile_frags(160) == [5, 5]
    assert su.split_tile_frags(240) == [8, 7]
    assert su.split_tile_frags(128) == [8] and su.split_tile_frags(132) == [5, 4]
    assert su.split_tile_frags(272) == [6, 6, 5] and su.split_tile_frags(720) == [8, 8, 8, 8, 8, 5]
    for W in range(4, 1025, 4):
        fr = su.split_tile_frags(W)
        assert sum(fr) == (W + 15) // 16 and max(fr) <= 8 and len(fr) == ((W + 15) // 16 + 7) // 8


def test_split_sweep_covers_every_fragment_pair_and_tail():
    """All 64 (fa, fb) of build_split_kernel's run-time switch, each with
    every column tail W % 16 on either side, where the tile with the tail is
    the one counted."""
    seen = {}
    for band in su.SPLIT_CROSS_BANDS:
        for W1 in band:
            for W2 in su.M4:
                key = (su.split_tile_frags(W1)[-1], su.split_tile_frags(W2)[-1])
                seen.setdefault(key, set()).add((W1 % 16, W2 % 16))
    want = {(a, b) for a in TAILS16 for b in TAILS16}
    for fa in range(1, 9):
        for fb in range(1, 9):
            assert seen.get((fa, fb)) == want, (fa, fb)
    # the first two-tile widths, and the balanced sweep's tile counts
    assert any(len(su.split_tile_frags(w)) == 2 for w in su.M4)
    assert {len(su.split_tile_frags(w)) for w in su.BAL_W + su.BAL_EXTRA} == {2, 3, 6}
    # two balanced tiles of 5..8 fragments, equal and with a shorter last tile
    frs = [su.split_tile_frags(w) for w in su.BAL_W]
    assert {f[0] for f in frs} == {5, 6, 7, 8} and {f[0] - f[1] for f in frs} == {0, 1}
    assert {w % 16 for w in su.BAL_W} == TAILS16


# the table of test_volume_sweep_gpu.py's docstring
RING_TABLE = {
    (False, (2, 4)): "65-128", (False, (2, 5)): "129-160", (False, (3, 4)): "161-192, 321-384",
    (False, (3, 5)): "193-240, 385-480, 641-720", (False, (4, 4)): "241-256, 481-512, 721-768",
    (False, (4, 5)): "257-320",
    (True, (2, 4)): "65-128", (True, (3, 4)): "129-192", (True, (4, 4)): "193-256", (True, (5, 4)): "257-320",
}


def test_ring_shape_restatement_matches_table():
    """csrc/volume.hip, bf16_ring_shape, over W2 = 65..768 (deferred: to 320,
    the widest its five 64-column waves hold in one tile)."""
    got = {}
    for W2 in range(65, 769):
        got.setdefault((False, su.bf16_ring_shape(W2, 72, False)), []).append(W2)
        if W2 <= 320:
            got.setdefault((True, su.bf16_ring_shape(W2, 72, True)), []).append(W2)
    table = {k: su.ranges(v) for k, v in got.items()}
    # 513-640 fall to instances the table lists by their first ranges only
    for key, text in RING_TABLE.items():
        have = [r for r in table[key].split(", ") if not 513 <= int(r.split("-")[0]) <= 640]
        assert ", ".join(have) == text, (key, table[key])
    assert su.bf16_ring_shape(64, 72, False) is None and su.bf16_ring_shape(100, 32, False) is None
    assert su.bf16_ring_shape(100, 33, False) == (2, 4)


def test_bf16_sweeps_cover_every_ring_instance():
    plain = {su.bf16_ring_shape(w, su.BF16_D, False) for w in su.BF16_W2}      # forms b (3-level) and c (5-level)
    defer = {su.bf16_ring_shape(w, su.BF16_D, True) for w in su.BF16_W2}       # form a
    assert plain == set(su.B16_PLAIN) and defer == set(su.B16_DEFER)
    # every band meets more than one instance boundary or lies inside one: none is empty
    assert all(su.BF16_W2_BANDS) and sum(map(len, su.BF16_W2_BANDS)) == 336
    # the second and third ranges of (4,4)
    wide = {su.bf16_ring_shape(w, su.BF16_D, False) for w in su.BF16_W2_WIDE}
    assert wide == {(4, 4)}
    assert {w for w in su.BF16_W2_WIDE if w <= 512} and {w for w in su.BF16_W2_WIDE if w >= 721}
    # the D sweep: one W2 per instance, every D on the ring
    assert [su.bf16_ring_shape(w, 64, False) for w in su.BF16_D_PLAIN_W2] == \
        [(2, 4), (2, 5), (3, 4), (3, 5), (4, 4), (4, 5)]
    assert [su.bf16_ring_shape(w, 64, True) for w in su.BF16_D_DEFER_W2] == [(2, 4), (3, 4), (4, 4), (5, 4)]
    assert all(su.bf16_ring_shape(311, D, False) for D in su.BF16_DS)
    # the last 32-row stage: full, one row, 8 valid rows, ...
    assert {D % 32 for D in su.BF16_DS} >= {0, 1, 8, 31}
    # the W1 sweep: the idle second wave row (W1 < 64), the 128-row tile and its tails
    assert min(su.BF16_W1) == 1 and max(su.BF16_W1) > 256
    assert {su.bf16_ring_shape(w, su.BF16_D, True) for w in su.BF16_W1_W2} == {(2, 4), (5, 4)}
    # the per-wave list stays below the ring's limits, in both aligned forms
    assert all(su.bf16_ring_shape(W2, D, False) is None for D, _, W2 in su.BF16_PERWAVE)
    assert {(W1 % 8 == 0 and W2 % 8 == 0) for _, W1, W2 in su.BF16_PERWAVE} == {True, False}
    # records: one tile spans the row, ceil(W2 / 64) = 2..5 waves; D > 224
    assert {(w + 63) // 64 for w in su.REC_W2} == {2, 3, 4, 5} and min(su.REC_D) > 224
    assert min(su.REC_W2) > 64 and max(su.REC_W2) <= 320


def test_backward_sweeps_cover_every_k_tail():
    """The width is the reduction dimension of both backward GEMMs (32-wide k
    steps): every tail W % 32 of a multiple of 4, for W1 and for W2, in every
    layout of the split path; every tail at all on the exact path."""
    tails = set(range(0, 32, 4))
    for layout in su.BWD_LAYOUTS:
        ok = [(a, b) for a, b in su.BWD_SHAPES if su.bwd_layout_ok(layout, b)]
        assert {a % 32 for a, _ in ok} == tails and {b % 32 for _, b in ok} == tails, layout
        for p in su.BWD_PARTNERS:                     # each partner meets every tail in both roles
            assert {b % 32 for a, b in ok if a == p} == tails, (layout, p)
            if su.bwd_layout_ok(layout, p):
                assert {a % 32 for a, b in ok if b == p} == tails, (layout, p)
    assert {w % 32 for w in su.BWD_EXACT_W2} == set(range(32)) == {w % 32 for w in su.BWD_EXACT_W1}
    # D is the output dimension: 128-row tiles, 16-row fragments
    assert {D % 16 for D in su.BWD_DS} >= {0, 1, 15} and max(su.BWD_DS) > 128
    assert [w1 % 4 == 0 and w2 % 4 == 0 for w1, w2 in su.BWD_D_SHAPES] == [True, True, False]


def test_exact_sweeps_select_their_kernels():
    """rc_launch_build_f32: the vector ring for widths multiples of 4 on both
    sides, else build_f32_kernel<false, ..>."""
    assert all(w1 % 4 == 0 and w2 % 4 == 0 for w1, w2 in su.EXACT_VEC_SHAPES)
    assert 21 % 4 and 37 % 4                                        # the any-width sweeps' fixed sides
    assert all(w1 % 4 == 0 and w2 % 4 == 0 for w1, w2 in su.DISP_SHAPES)
    assert su.max_nbuf(1, 5) == 1 and su.max_nbuf(15, 5) == 4 and su.max_nbuf(16, 5) == 5


# ------------------------------------------------------------- sensitivity

def perturbed(ref):
    """Two copies of a 2-D oracle output with one small defect each, in the
    middle row: (1) one element replaced by its row neighbour's value, at the
    adjacent pair whose difference is the row's median (a typical pair, not
    the worst); (2) that pair swapped.  A single column has no row
    neighbours: the pair is then taken down the column."""
    a = np.array(ref, np.float32)
    if a.shape[1] == 1:
        a = a.T
    row = a.shape[0] // 2
    d = np.abs(np.diff(a[row]))
    assert d.size, "no neighbour to take a value from"
    j = int(np.argsort(d)[d.size // 2])
    one, swap = a.copy(), a.copy()
    one[row, j] = a[row, j + 1]
    swap[row, j], swap[row, j + 1] = a[row, j + 1], a[row, j]
    back = (lambda x: x.T) if np.shape(ref)[1] == 1 else (lambda x: x)
    return back(one), back(swap)


def volume(D, H, W1, W2, bf16=False):
    g = torch.Generator().manual_seed(D + W1 + W2)
    f1, f2 = torch.randn(1, D, H, W1, generator=g), torch.randn(1, D, H, W2, generator=g)
    if bf16:
        f1, f2 = f1.bfloat16().float(), f2.bfloat16().float()
    return coracle.corr_volume(f1.numpy(), f2.numpy()).reshape(H * W1, W2)


def fails_f32(a, ref):
    return norm_err(a, ref) > 1e-4 or rel_l2(a, ref) > 1e-5


# (sweep, bound, the smallest and the largest shape as (D, H, W1, W2))
VOLUME_SWEEPS = [
    ("bf16 W2, fp32 pyramid", 1e-5, [(72, 2, 24, 65), (72, 1, 24, 400)]),
    ("bf16 W2, bf16 pyramid", 8e-3, [(72, 2, 24, 65), (72, 1, 24, 400)]),
    ("bf16 wide, fp32 pyramid", 1e-5, [(72, 1, 24, 481), (72, 1, 24, 768)]),
    ("bf16 W1, fp32 pyramid", 1e-5, [(72, 2, 1, 70), (72, 1, 260, 311)]),
    ("bf16 W1, bf16 pyramid", 8e-3, [(72, 2, 1, 70), (72, 1, 260, 311)]),
    ("bf16 D, fp32 pyramid", 1e-5, [(33, 1, 40, 100), (264, 2, 40, 311)]),
    ("bf16 D, bf16 pyramid", 8e-3, [(33, 1, 40, 100), (264, 2, 40, 311)]),
    ("bf16 per-wave, fp32 pyramid", 1e-5, [(1, 1, 37, 100), (8, 1, 37, 8), (72, 2, 40, 64)]),
    ("bf16 per-wave, bf16 pyramid", 8e-3, [(1, 1, 37, 100), (8, 1, 37, 8), (72, 2, 40, 64)]),
    ("f32 fmaps, bf16 pyramid", 8e-3, [(40, 1, 20, 2), (40, 1, 20, 140), (40, 2, 1, 36), (40, 1, 140, 36)]),
    ("records", 8e-3, [(225, 1, 8, 65), (256, 1, 70, 320)]),
    ("split fragment pairs", None, [(40, 1, 4, 4), (40, 1, 132, 132)]),
    ("split balanced tiles", None, [(40, 1, 132, 16), (40, 1, 720, 240)]),
    ("split D states", None, [(1, 1, 20, 36), (256, 1, 132, 72), (17, 514, 16, 16)]),
    ("exact any width", None, [(40, 1, 21, 1), (40, 1, 21, 140), (40, 1, 1, 37), (40, 1, 140, 37)]),
    ("exact vector ring", None, [(40, 1, 4, 4), (40, 1, 144, 132)]),
]


@pytest.mark.parametrize("sweep", VOLUME_SWEEPS, ids=lambda s: s[0].replace(" ", "_").replace(",", ""))
def test_volume_bounds_notice_one_wrong_element(sweep):
    name, tol, shapes = sweep
    for D, H, W1, W2 in shapes:
        ref = volume(D, H, W1, W2, bf16=tol is not None)
        assert not (fails_f32(ref, ref) if tol is None else norm_err(ref, ref) > tol)
        for bad in perturbed(ref):
            caught = fails_f32(bad, ref) if tol is None else norm_err(bad, ref) > tol
            assert caught, (name, D, H, W1, W2)


BACKWARD_SWEEPS = [
    ("split widths", [(40, 1, 4, 4, 1), (40, 2, 132, 132, 3)]),
    ("exact widths", [(40, 2, 21, 1, 1), (40, 1, 21, 140, 3), (40, 1, 1, 37, 3), (40, 2, 140, 37, 3)]),
    ("D", [(1, 1, 36, 40, 3), (256, 1, 311, 311, 3)]),
]


@pytest.mark.parametrize("sweep", BACKWARD_SWEEPS, ids=lambda s: s[0].replace(" ", "_"))
def test_backward_bounds_notice_one_wrong_element(sweep):
    name, shapes = sweep
    for D, H, W1, W2, nlev in shapes:
        g = torch.Generator().manual_seed(D + W1 + W2)
        f1, f2 = torch.randn(1, D, H, W1, generator=g), torch.randn(1, D, H, W2, generator=g)
        grads = [torch.randn(H * W1, W2 >> l, generator=g).numpy() for l in range(nlev)]
        for ref in coracle.corr_build_backward(f1.numpy(), f2.numpy(), grads):
            ref = ref.reshape(D * H, -1)
            if ref.size == 1:
                continue                                  # a single value has no neighbour
            assert not fails_f32(ref, ref)
            for bad in perturbed(ref):
                assert fails_f32(bad, ref), (name, D, H, W1, W2)


# ------------------------------------------------------------------- arena

def test_sentinels_are_nan():
    assert np.isnan(np.array([su.SENT32], np.uint32).view(np.float32)[0])
    assert np.isnan(np.array([su.SENT16 << 16 | su.SENT16], np.uint32).view(np.float32)[0])
    assert np.isnan(su.bf16_to_f32(np.array([su.SENT16], np.uint16))[0])


@pytest.mark.parametrize("phase", [0, 1])
@pytest.mark.parametrize("base", [0, 512, 16, 4096 + 48, 112])
def test_plan_offsets_phases_and_guards(base, phase):
    sizes = [4, 6, 16, 100, 4096, 4097, 12345, 2]
    offs, total = su.plan(sizes, base, phase)
    assert total <= su.bound(sizes) and total % 4 == 0
    end = 0
    for i, (o, n) in enumerate(zip(offs, sizes)):
        assert (base + o) % 128 == su.PHASES[(phase + i) % 2]
        assert (base + o) % 16 == 0 and (base + o) % 128 != 0
        assert o - end >= su.GUARD
        end = o + n
    assert total - end >= su.GUARD
    assert {(base + o) % 128 for o in offs} == set(su.PHASES)


def make_arena(bf16=False, phase=0):
    a = torch.arange(50, dtype=torch.float32)
    b = torch.arange(33, dtype=torch.float32).bfloat16()
    specs = [("a", 200, a), ("out", 404, None), ("b", 66, b), ("out2", 2, None)]
    return su.arena("cpu", specs, phase, bf16), a, b


@pytest.mark.parametrize("bf16", [False, True])
def test_arena_bookkeeping(bf16):
    ar, a, b = make_arena(bf16, 1)
    names = ["a", "out", "b", "out2"]
    for i, n in enumerate(names):
        assert ar.ptr(n) % 128 == su.PHASES[(1 + i) % 2] and ar.ptr(n) == ar.base + ar.off[n]
    order = sorted(names, key=lambda n: ar.off[n])
    assert order == names and ar.off["a"] >= su.GUARD
    for p, q in zip(order, order[1:]):
        assert ar.off[q] - (ar.off[p] + ar.size[p]) >= su.GUARD
    assert ar.total - (ar.off["out2"] + ar.size["out2"]) >= su.GUARD
    assert ar.outputs == ["out", "out2"]
    # inputs are what was written; everything else is the sentinel
    assert torch.equal(ar.tensor("a", torch.float32, (50,)), a)
    assert torch.equal(ar.tensor("b", torch.bfloat16, (33,)), b)
    img = ar.fetch().copy()
    for n in ("a", "b"):
        img[ar.off[n]:ar.off[n] + ar.size[n]] = 0
    sent = np.array([ar.sent], np.uint32).view(np.uint8)
    rest = np.ones(img.size, bool)
    for n in ("a", "b"):
        rest[ar.off[n]:ar.off[n] + ar.size[n]] = False
    assert (img.reshape(-1, 4)[rest.reshape(-1, 4).all(1)] == sent).all()
    assert np.isnan(ar.region("out", np.float32)).all()
    ar.assert_guards_intact()


def test_arena_guards_notice_every_stray_write():
    def poke(name, delta, end):
        ar, _, _ = make_arena()
        at = ar.off[name] + (ar.size[name] if end else 0) + delta
        ar.buf.view(torch.uint8)[at] ^= 1
        return ar

    for name in ("a", "out", "b", "out2"):
        for delta, end in ((-1, False), (-su.GUARD, False), (0, True), (su.GUARD - 1, True)):
            with pytest.raises(AssertionError, match="guard overwritten"):
                poke(name, delta, end).assert_guards_intact()
    for name in ("a", "b"):                               # an input is read-only
        for delta, end in ((0, False), (-1, True)):
            with pytest.raises(AssertionError, match=f"input {name} modified"):
                poke(name, delta, end).assert_guards_intact()
    for name in ("out", "out2"):                          # an output may change, every byte of it
        for delta, end in ((0, False), (-1, True)):
            poke(name, delta, end).assert_guards_intact()
    ar, _, _ = make_arena()
    ar.buf.view(torch.uint8)[ar.total - 1] ^= 1           # the last byte of the trailing guard
    with pytest.raises(AssertionError):
        ar.assert_guards_intact()
    ar, _, _ = make_arena()
    ar.buf.view(torch.uint8)[0] ^= 1                      # the first byte of the leading guard
    with pytest.raises(AssertionError):
        ar.assert_guards_intact()
