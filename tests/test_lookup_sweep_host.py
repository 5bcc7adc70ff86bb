"""Host-side companion of test_lookup_sweep_gpu.py (no GPU): the CPU pyramids
hold the pool chain, the arena's in/out regions and assert_outputs_written
keep their books, and the sweep lists reach the residues, tails and kernel
instances the GPU file's docstring claims."""
import numpy as np
import pytest
import torch

import lookup_sweep_util as lsu
import sweep_util as su
from golden_util import same
from oracle import coracle
from raft_stereo_amd import _lib


# ------------------------------------------------------------ CPU pyramid

@pytest.mark.parametrize("kind", lsu.KINDS)
def test_cpu_pyramid_holds_the_pool_chain(kind):
    for W2, L in ((143, 4), (16, 4), (8, 4), (67, 2), (3, 2), (37, 5), (2, 1)):
        pyr = lsu.cpu_pyramid(37, W2, L, kind, W2)
        assert [p.shape for p in pyr] == [(37, W2 >> l) for l in range(L)]
        assert same(pyr[0], lsu.round_kind(pyr[0], kind)), "level 0 is not of the element type"
        assert np.isfinite(pyr[0]).all() and np.abs(pyr[0]).max() > 1
        for l in range(1, L):
            a, b = pyr[l - 1][:, 0:2 * (W2 >> l):2], pyr[l - 1][:, 1:2 * (W2 >> l):2]
            want = lsu.round_kind((a + b) * np.float32(0.5), kind)
            assert same(pyr[l], want), (kind, W2, l)
            assert same(pyr[l], lsu.round_kind(pyr[l], kind))
    # fp32: the oracle's pooling is the reference's (model.py:294)
    assert same(lsu.cpu_pyramid(5, 21, 3, "f32", 1)[2], coracle.corr_pool(coracle.corr_pool(
        lsu.cpu_pyramid(5, 21, 3, "f32", 1)[0])))
    # a different seed is a different pyramid
    assert not same(lsu.cpu_pyramid(5, 21, 1, "f32", 1)[0], lsu.cpu_pyramid(5, 21, 1, "f32", 2)[0])


@pytest.mark.parametrize("kind", lsu.KINDS)
@pytest.mark.parametrize("shadow", [False, True])
def test_level_image_pads_and_poisons(kind, shadow):
    """Rows padded to 16 bytes, the padding and the gap before the shadow copy
    the NaN pattern, the values' bits in place in both copies."""
    bf = kind != "f32"
    P, W = 5, 21
    lvl = lsu.cpu_pyramid(P, W, 1, kind, 3)[0]
    t, ld = lsu.level_image(lvl, kind, bf, shadow)
    es = lsu.ES[kind]
    assert ld * es % 16 == 0 and W <= ld < W + 16 // es
    raw = t.numpy().view(np.uint16 if es == 2 else np.uint32)
    sent = su.SENT16 if es == 2 else su.SENT32
    back = (lambda u: su.bf16_to_f32(u)) if kind == "bf16" else \
        (lambda u: u.view(np.float16).astype(np.float32)) if kind == "f16" else (lambda u: u.view(np.float32))
    offs = [0] + ([_lib.shadow_offset(P, ld, es) // es] if shadow else [])
    assert raw.size == offs[-1] + P * ld
    keep = np.zeros(raw.size, bool)
    for o in offs:
        rows = raw[o:o + P * ld].reshape(P, ld)
        assert same(back(np.ascontiguousarray(rows[:, :W])), lvl)
        assert (rows[:, W:] == sent).all()
        keep[o:o + P * ld] = True
    assert (raw[~keep] == sent).all() and (not shadow or (~keep).sum() * es >= 64)
    assert np.isnan(back(np.array([sent], raw.dtype)))[0]


def test_coords_image_poisons_y():
    x = np.arange(6, dtype=np.float32).reshape(1, 2, 3)
    for bf in (False, True):
        c = lsu.coords_image(x, bf).numpy().view(np.float32)
        assert same(c[:, 0], x) and np.isnan(c[:, 1]).all()
        assert (c[:, 1].view(np.uint32) == lsu.sent32(bf)).all()


def test_coord_sets_hold_what_the_docstring_says():
    for (B, H, W1), W2 in zip(lsu.SHAPES, (16, 37, 143, 2)):
        cs = lsu.coord_sets(B, H, W1, W2, 5)
        sp = cs["special"][0]
        assert all(x.shape == (B, H, W1) and x.dtype == np.float32 for x in lsu.all_sets(cs))
        assert np.isnan(sp).any() and np.isposinf(sp).any() and np.isneginf(sp).any()
        assert (sp == np.float32(1e30)).any() and (sp == np.float32(-1e30)).any()
        assert (sp[sp == 0].view(np.uint32) == 0x80000000).any() and (sp[sp == 0].view(np.uint32) == 0).any()
        sweep = np.concatenate([x.reshape(-1) for x in cs["sweep"]])
        for k in range(-40, W2 + 41):
            f = np.float32(k)
            for v in (f, np.nextafter(f, np.float32(np.inf)), np.nextafter(f, np.float32(-np.inf))):
                assert (sweep == v).any(), (W2, k)
        assert all(np.isfinite(x).all() for x in lsu.finite_sets(cs))
        sm = cs["smooth"][0]
        assert sm.min() > -8 and sm.max() < W2 + 4 and np.abs(np.diff(sm, axis=2)).max() < max(4.0, 2 * W2 / W1 + 2)
    big = lsu.packed_coords(1, 937, 70, 16, 0)
    assert big.shape == (1, 937, 70) and np.isnan(big).any() and (big == 56.0).any()


# ------------------------------------------------------------------ arena

def make_arena(bf16=False):
    a = torch.arange(50, dtype=torch.float32)
    g = torch.arange(24, dtype=torch.float32)
    specs = [("a", 200, a), ("out", 404, None), ("g", 96, g, True), ("h", 66, None)]
    return su.arena("cpu", specs, 0, bf16), a, g


@pytest.mark.parametrize("bf16", [False, True])
def test_inout_region_bookkeeping(bf16):
    """An in/out region carries its initial data and may change; a 3-tuple
    spec still means what it meant."""
    ar, a, g = make_arena(bf16)
    assert ar.outputs == ["out", "g", "h"]
    assert torch.equal(ar.tensor("g", torch.float32, (24,)), g)
    assert torch.equal(ar.tensor("a", torch.float32, (50,)), a)
    ar.assert_guards_intact()
    ar.tensor("g", torch.float32, (24,))[3] += 1.0           # the "kernel" accumulates
    ar.buf.view(torch.uint8)[ar.off["g"] + 95] ^= 1           # ... into the last byte too
    ar.assert_guards_intact()
    ar.buf.view(torch.uint8)[ar.off["a"]] ^= 1                # an input stays read-only
    with pytest.raises(AssertionError, match="input a modified"):
        ar.assert_guards_intact()
    with pytest.raises(AssertionError):
        su.arena("cpu", [("x", 8, None, True)])               # in/out without data


@pytest.mark.parametrize("name", ["g", "out"])
def test_one_byte_past_a_region_is_caught(name):
    for delta in (0, su.GUARD - 1):
        ar, _, _ = make_arena()
        ar.buf.view(torch.uint8)[ar.off[name] + ar.size[name] + delta] ^= 1
        with pytest.raises(AssertionError, match="guard overwritten"):
            ar.assert_guards_intact()
    ar, _, _ = make_arena()
    ar.buf.view(torch.uint8)[ar.off[name] - 1] ^= 1
    with pytest.raises(AssertionError, match="guard overwritten"):
        ar.assert_guards_intact()


@pytest.mark.parametrize("bf16", [False, True])
def test_assert_outputs_written(bf16):
    """A hand-made kernel that writes every element passes; one that leaves a
    single element unwritten is caught, for 4-byte and for 2-byte elements,
    also where the reference would be NaN."""
    ar, _, _ = make_arena(bf16)
    with pytest.raises(AssertionError, match="output out: 101 of 101 elements never written"):
        ar.assert_outputs_written(["out"])
    out = ar.tensor("out", torch.float32, (101,))
    out.copy_(torch.arange(101.0))
    out[7] = float("nan")                                     # a NaN the kernel computed is a written element
    ar.fetch()
    ar.assert_outputs_written(["out"])
    ar.tensor("out", torch.int32, (101,))[100] = ar.sent     # the last element left unwritten
    ar.fetch()
    with pytest.raises(AssertionError, match="1 of 101 elements never written, the first at index 100"):
        ar.assert_outputs_written(["out"])
    with pytest.raises(AssertionError, match="not an output region"):
        ar.assert_outputs_written(["a"])
    if bf16:                                                  # 2-byte elements: 33 of them in "h"
        h = ar.tensor("h", torch.bfloat16, (33,))
        h.copy_(torch.arange(33.0))
        ar.fetch()
        ar.assert_outputs_written(["h"], 2)
        ar.tensor("h", torch.int16, (33,))[32] = su.SENT16
        ar.fetch()
        with pytest.raises(AssertionError, match="1 of 33 elements never written, the first at index 32"):
            ar.assert_outputs_written(["h"], 2)
        # 0x7FC1 is a NaN as fp16 too
        assert np.isnan(np.array([su.SENT16], np.uint16).view(np.float16)[0])
    # an in/out region holds data from the start: nothing to find
    ar.assert_outputs_written(["g"])


# --------------------------------------------------------------- coverage

def test_shapes_are_the_docstrings():
    assert [b * h * w for b, h, w in lsu.SHAPES] == [37, 74, 140, 280]
    assert {b for b, _, _ in lsu.SHAPES} == {1, 2} == {h for _, h, _ in lsu.SHAPES}
    assert 280 > 256 and 280 % 256 == 24 and 37 < 64 < 74
    # every band of 16 consecutive widths meets all four shapes
    assert {lsu.shape_for(w) for w in range(16, 32)} == set(lsu.SHAPES)


def test_pair_sweep_residues():
    """Part a: every residue of W2 mod 64 (L = 4), so of the level-0 and
    level-2 widths mod 16; odd widths at every level; each 16-bit type at
    every residue of W2 mod 32, odd widths included; r = 2, 3 at eight widths
    each, inside the sweep."""
    assert lsu.PAIR4_W2 == list(range(16, 144)) and lsu.PAIR2_W2 == list(range(4, 68))
    assert {w % 64 for w in lsu.PAIR4_W2} == set(range(64)) == {w % 64 for w in lsu.PAIR2_W2}
    assert {w % 16 for w in lsu.PAIR4_W2} == set(range(16)) == {(w >> 2) % 16 for w in lsu.PAIR4_W2}
    for l in range(4):
        assert any((w >> l) % 2 for w in lsu.PAIR4_W2)
    assert sum(lsu.PAIR_BANDS[4], []) == lsu.PAIR4_W2 and sum(lsu.PAIR_BANDS[2], []) == lsu.PAIR2_W2
    for widths in (lsu.PAIR4_W2, lsu.PAIR2_W2):
        for kind in ("bf16", "f16"):
            mine = [w for w in widths if kind in lsu.pair_kinds(w)]
            assert len(mine) == len(widths) // 2 and {w % 32 for w in mine} == set(range(32)), kind
            assert any(w % 2 for w in mine) and any(w % 2 == 0 for w in mine)
        assert all("f32" in lsu.pair_kinds(w) for w in widths)
    for L, widths in ((4, lsu.PAIR4_W2), (2, lsu.PAIR2_W2)):
        for r in (2, 3):
            ws = lsu.PAIR_MID_R[L][r]
            assert len(set(ws)) == 8 and set(ws) <= set(widths) and any(w % 2 for w in ws)
    # the smallest widths keep every looked-up level at width >= 2
    assert min(lsu.PAIR4_W2) >> 3 == 2 and min(lsu.PAIR2_W2) >> 1 == 2
    assert all(lsu.chain_kernel(4, (0, 2)) == "pair" == lsu.chain_kernel(2, (0,)) for _ in (0,))


def test_channels_last_tail_residues():
    """(P % 64) * C of the tail cases: every residue in {2, 4, 6} mod 8 (the
    16-bit outputs' vectors of 8) and residue 2 mod 4 (fp32, vectors of 4)."""
    assert [w % 64 for w in lsu.CL_TAIL_W1] == [1, 37]
    Cs = {2: [2 * (2 * r + 1) for r in (1, 2, 3, 4)], 4: [4 * (2 * r + 1) for r in (1, 2, 3, 4)]}
    assert Cs == {2: [6, 10, 14, 18], 4: [12, 20, 28, 36]}
    tails8 = {lsu.cl_tail(P, C, 2) for P in lsu.CL_TAIL_W1 for L in (2, 4) for C in Cs[L]}
    tails4 = {lsu.cl_tail(P, C, 4) for P in lsu.CL_TAIL_W1 for L in (2, 4) for C in Cs[L]}
    assert tails8 == {2, 4, 6} and tails4 == {0, 2}
    for P in lsu.CL_TAIL_W1:                                  # each P alone reaches them too
        assert {lsu.cl_tail(P, C, 2) for L in (2, 4) for C in Cs[L]} == {2, 4, 6}
    # the main sweep's shapes: partial last waves of 37, 10, 12 and 24 pixels
    assert [b * h * w % 64 for b, h, w in lsu.SHAPES] == [37, 10, 12, 24]
    assert lsu.CL_TAIL_W2[4] >> 3 >= 2 and lsu.CL_TAIL_W2[2] >> 1 >= 2


def test_chain_and_level_sweeps_select_their_kernels():
    assert lsu.CHAIN_W2[4] == list(range(16, 80)) and lsu.CHAIN_W2[3] == list(range(8, 72))
    assert lsu.chain_kernel(4, (0, 1)) == "level1_chain" == lsu.chain_kernel(3, (0, 1))
    assert lsu.chain_kernel(3, (0, 2)) is None and lsu.chain_kernel(4, (0,)) is None
    assert min(lsu.CHAIN_W2[4]) >> 3 == 2 and min(lsu.CHAIN_W2[3]) >> 2 == 2
    for L in range(1, 6):
        ws = lsu.level_w2(L)
        assert len(ws) == 16 and ws[0] == 1 << L and ws[-1] == (1 << L) + 70
        assert any(w % 2 for w in ws) and any(w % 2 == 0 for w in ws) and ws[0] >> (L - 1) == 2
        for b, h, w in lsu.SHAPES:
            assert lsu.level_kernel(b * h * w, L, "f32") == ("levelpar" if L <= 4 else "runtime_loop")
            assert lsu.level_kernel(b * h * w, L, "f16") == "f16pyr_level"
    # the two thresholds (csrc/lookup.hip: kLevelParP, kSmallP)
    assert (lsu.LEVELPAR_P, lsu.SMALL_P) == (65536, 131072)
    got = [lsu.level_kernel(b * h * w, 4, "f32") for b, h, w in lsu.LARGE_P]
    assert got == ["unrolled64", "runtime_loop"]
    assert [b * h * w for b, h, w in lsu.LARGE_P] == [65590, 131110]
    src = open(_lib.HEADER.replace("include/raftcorr.h", "raft-stereo_amd/csrc/lookup.hip")).read()
    assert "kSmallP = 256LL * 256 * 2" in src and "kLevelParP = 64LL * 1024" in src


def test_layout_and_backward_lists():
    assert len(lsu.DISP_LOOKUP) == len(set(lsu.DISP_LOOKUP)) == 16 and set(lsu.DISP_LOOKUP) <= set(su.DISP_SHAPES)
    assert all(w2 >> 3 >= 2 for _, w2 in lsu.DISP_LOOKUP)
    assert lsu.REC_LOOKUP_W2[0] == su.REC_W2[0] and lsu.REC_LOOKUP_W2[-1] == su.REC_W2[-1]
    assert len(lsu.REC_LOOKUP_W2) == 8 and set(lsu.REC_LOOKUP_W2) <= set(su.REC_W2)
    for ws, n in ((lsu.STEP_W2, 8), (lsu.CONV_W2, 12), (lsu.BWD_W2, 16), (lsu.CALLS_W2, 8)):
        assert len(set(ws)) == n and set(ws) <= set(lsu.PAIR4_W2) and any(w % 2 for w in ws)
    # the gradient rows: every W mod 4, dense rows (W % 4 == 0) included, at levels 0 and 2
    assert {w % 4 for w in lsu.BWD_W2} == {0, 1, 2, 3} == {(w >> 2) % 4 for w in lsu.BWD_W2}
    assert any(su.grad_ld(w) == w for w in lsu.BWD_W2) and any(su.grad_ld(w) > w for w in lsu.BWD_W2)
    # the 256-pixel workgroup partials: 1, 1, 2 and 3 workgroups
    Ps = [b * h * w for b, h, w in lsu.CONV_BWD_P]
    assert Ps == [37, 256, 257, 513] and [(p + 255) // 256 for p in Ps] == [1, 1, 2, 3]
    assert _lib.lookup_conv_bwd_ws(257, 3, 36) == 2 * 3 * 37
