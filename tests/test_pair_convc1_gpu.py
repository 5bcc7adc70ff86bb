"""The fused lookup + convc1 on the stored pair levels
(rc_corr_lookup_chain_conv / _backward, ``CorrBlock1D.lookup_convc1`` on a
default block): bit-identical to the per-level fused kernels
on the full pyramid, forward and backward, with nothing pooled into memory;
fp16 / bf16 output equal to the cast of the fp32 output bit for bit; autograd
through the block; the routes that keep the per-level kernel; the network
option.

Coordinates are ``special_coords`` of test_corr_gpu.py: NaN, +-inf, +-1e30,
subnormal x, a sweep across both row edges and in-range pixels."""
import functools

import pytest
import torch
import torch.nn.functional as F

from golden_util import norm_err
from raft_stereo_amd import CorrBlock1D
from raft_stereo_amd import corr as rcorr
from test_corr_gpu import special_coords

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5            # the project's fp32 bound (MIOpen sums in another order)
BF16, FP16 = torch.bfloat16, torch.float16

SHAPES = [
    # B, D, H, W1, W2, L, r, cout
    (1, 8, 1, 20, 16, 4, 1, 8),        # P = 20 < one wave; level 3 of width 2
    (2, 16, 3, 57, 240, 4, 4, 64),     # P = 342: second workgroup partial; W1 != W2
    (1, 8, 2, 33, 64, 2, 2, 1),        # two levels; cout = 1
    (2, 32, 3, 130, 130, 4, 4, 63),    # P = 780: four workgroups; odd cout; padded row stride
    (1, 16, 2, 45, 61, 4, 2, 64),      # odd W2 > W1
    (2, 64, 5, 96, 96, 4, 4, 64),      # also with a bf16 pyramid
    (1, 32, 2, 311, 311, 4, 3, 16),    # bf16 pyramid; KITTI's width
]
# (shape, pyramid dtype, shadow): None = the block's default shadow levels
CASES = [
    (SHAPES[0], None, None),
    (SHAPES[1], None, True), (SHAPES[1], None, False),
    (SHAPES[2], None, None),
    (SHAPES[3], None, None),
    (SHAPES[4], None, None),
    (SHAPES[5], None, True), (SHAPES[5], None, False),
    (SHAPES[5], BF16, True), (SHAPES[5], BF16, False),
    (SHAPES[6], BF16, None),
]
IDS = ["x".join(map(str, s)) + ("-bf16" if pd else "") + ({None: "", True: "-shadow", False: "-noshadow"}[sh])
       for s, pd, sh in CASES]
case = pytest.mark.parametrize("case", CASES, ids=IDS)


def same_bits(a, b):
    """NaN at the same positions, the same bits everywhere else."""
    assert a.dtype == b.dtype and a.shape == b.shape
    na, nb = torch.isnan(a), torch.isnan(b)
    if not torch.equal(na, nb):
        return False
    iv = torch.int32 if a.element_size() == 4 else torch.int16
    return torch.equal(a.contiguous().view(iv)[~na], b.contiguous().view(iv)[~nb])


@functools.lru_cache(maxsize=None)
def inputs(shape):
    B, D, H, W1, W2, L, r, cout = shape
    g = torch.Generator().manual_seed(4100 + sum(shape))
    cin = L * (2 * r + 1)
    f1 = torch.randn(B, D, H, W1, generator=g).to(DEV)
    f2 = torch.randn(B, D, H, W2, generator=g).to(DEV)
    coords = special_coords(B, H, W1, W2, g)
    # the same field with the non-finite and huge entries replaced: gradient
    # sums over all pixels that are not NaN throughout
    x = coords[:, :1].clone()
    bad = ~torch.isfinite(x) | (x.abs() > 1e6)
    x[bad] = 3.25
    finite = torch.cat([x, torch.zeros_like(x)], 1)
    W = (torch.randn(cout, cin, generator=g) / cin ** 0.5).to(DEV)
    b = (torch.randn(cout, generator=g) * 0.1).to(DEV)
    gout = torch.randn(B, cout, H, W1, generator=g).to(DEV)
    return dict(f1=f1, f2=f2, coords=coords.to(DEV), finite=finite.to(DEV), W=W, b=b, gout=gout)


def default_block(case, grad=False):
    shape, pd, sh = case
    inp = inputs(shape)
    f1, f2 = inp["f1"], inp["f2"]
    if grad:
        f1, f2 = f1.clone().requires_grad_(True), f2.clone().requires_grad_(True)
    blk = CorrBlock1D(f1, f2, num_levels=shape[5], radius=shape[6], pyramid_dtype=pd, shadow=sh)
    return blk, f1, f2


@functools.lru_cache(maxsize=None)
def full_pyramid(case):
    """Every level in memory, from a second, eager block: what the per-level
    kernels read."""
    shape, pd, _ = case
    inp = inputs(shape)
    with torch.no_grad():
        blk2 = CorrBlock1D(inp["f1"], inp["f2"], num_levels=shape[5], radius=shape[6], pyramid_dtype=pd,
                           lazy_levels=False)
    assert blk2.levels_stored == list(range(shape[5] + 1))
    return blk2.corr_pyramid


@functools.lru_cache(maxsize=None)
def per_level_forward(case, bias, relu):
    shape = case[0]
    inp = inputs(shape)
    with torch.no_grad():
        return rcorr.lookup_convc1(full_pyramid(case), inp["coords"], shape[5], shape[6], inp["W"],
                                   inp["b"] if bias else None, relu)


def stored_pair(L):
    return [0] if L == 2 else [0, 2]


@case
def test_forward_bit_identical_and_nothing_materialised(case):
    shape = case[0]
    L = shape[5]
    inp = inputs(shape)
    with torch.no_grad():
        blk, _, _ = default_block(case)
        assert blk.levels_stored == stored_pair(L)
        for bias in (True, False):
            for relu in (True, False):
                a = blk.lookup_convc1(inp["coords"], inp["W"], inp["b"] if bias else None, relu=relu)
                # the per-level path pools levels 1, 3 and 4 here
                assert blk.levels_stored == stored_pair(L), (bias, relu)
                assert a.dtype == torch.float32 and a.shape == (shape[0], shape[7], shape[2], shape[3])
                assert same_bits(a, per_level_forward(case, bias, relu)), (bias, relu)
        if case[2] is True:
            assert blk._shadow, "the shadowed case has no shadow copy"
        if case[2] is False:
            assert not blk._shadow


@case
@pytest.mark.parametrize("dt", [FP16, BF16], ids=["fp16", "bf16"])
def test_half_precision_output_is_the_cast(case, dt):
    shape = case[0]
    inp = inputs(shape)
    with torch.no_grad():
        blk, _, _ = default_block(case)
        for bias, relu in ((True, True), (True, False), (False, False)):   # without ReLU: the fused-convert hazard
            b = inp["b"] if bias else None
            h = blk.lookup_convc1(inp["coords"], inp["W"], b, relu=relu, out_dtype=dt)
            assert h.dtype == dt
            assert same_bits(h, per_level_forward(case, bias, relu).to(dt)), (bias, relu)
        f = blk.lookup_convc1(inp["coords"], inp["W"], inp["b"], out_dtype=torch.float32)
        assert f.dtype == torch.float32 and same_bits(f, per_level_forward(case, True, True))
        assert blk.levels_stored == stored_pair(shape[5])


@case
@pytest.mark.parametrize("relu", [True, False], ids=["relu", "norelu"])
def test_backward_bit_identical(case, relu):
    shape = case[0]
    L, r = shape[5], shape[6]
    inp = inputs(shape)
    with torch.no_grad():
        blk, _, _ = default_block(case)
        full = full_pyramid(case)
        for field in ("coords", "finite"):
            c = inp[field]
            args = (c, L, r, inp["W"], inp["b"], relu, inp["gout"])
            ref = rcorr.lookup_convc1_backward(full, *args)
            got = rcorr.lookup_chain_convc1_backward(blk._levels, *args, shadow=blk._shadow)
            again = rcorr.lookup_chain_convc1_backward(blk._levels, *args, shadow=blk._shadow)
            for name, x, y, z in zip(("grad_corr", "grad_weight", "grad_bias"), got, ref, again):
                assert same_bits(x, y), (field, name)
                assert same_bits(x, z), (field, name, "second run")
            if field == "finite":
                assert all(bool(torch.isfinite(t).all()) for t in got)
            # each gradient alone (the NULL combinations), and without a bias
            for i, need in enumerate(((True, False, False), (False, True, False), (False, False, True))):
                alone = rcorr.lookup_chain_convc1_backward(blk._levels, *args, *need, shadow=blk._shadow)
                assert [t is not None for t in alone] == list(need)
                assert same_bits(alone[i], ref[i]), (field, need)
            nb = (c, L, r, inp["W"], None, relu, inp["gout"])
            for x, y in zip(rcorr.lookup_chain_convc1_backward(blk._levels, *nb, need_bias=False,
                                                               shadow=blk._shadow)[:2],
                            rcorr.lookup_convc1_backward(full, *nb, need_bias=False)[:2]):
                assert same_bits(x, y), (field, "no bias")
        assert blk.levels_stored == stored_pair(L)


AUTOGRAD_CASES = [CASES[1], CASES[3], CASES[8]]


@pytest.mark.parametrize("case", AUTOGRAD_CASES, ids=[IDS[1], IDS[3], IDS[8]])
@pytest.mark.parametrize("dt", [None, FP16], ids=["fp32", "fp16"])
def test_autograd_through_the_block(case, dt):
    """df1, df2, dW, db of the new route equal those of the explicit
    composite ``lookup_convc1(...).to(dt)`` through the per-level kernels (an
    eager block whose pyramid is handed back to it, which selects the
    per-level route).  Bit-equal: grad_corr, grad_weight and grad_bias are
    (test_backward_bit_identical), the cast's backward is the same widening,
    and everything downstream of grad_corr is the same code on the same
    bits."""
    shape = case[0]
    L, r, cout = shape[5], shape[6], shape[7]
    inp = inputs(shape)
    go = inp["gout"] if dt is None else inp["gout"].to(dt)

    def run(new_route):
        blk, f1, f2 = default_block(case, grad=True) if new_route else (None, None, None)
        if not new_route:
            f1 = inp["f1"].clone().requires_grad_(True)
            f2 = inp["f2"].clone().requires_grad_(True)
            blk = CorrBlock1D(f1, f2, num_levels=L, radius=r, pyramid_dtype=case[1], lazy_levels=False)
            blk.corr_pyramid = blk.corr_pyramid          # a replaced pyramid: the per-level kernels
            assert not blk._chain
        W = inp["W"].clone().view(cout, -1, 1, 1).requires_grad_(True)
        b = inp["b"].clone().requires_grad_(True)
        if new_route:
            out = blk.lookup_convc1(inp["finite"], W, b, differentiable=True, out_dtype=dt)
        else:
            out = blk.lookup_convc1(inp["finite"], W, b, differentiable=True)
            out = out if dt is None else out.to(dt)
        assert out.dtype == (dt or torch.float32) and out.grad_fn is not None
        out.backward(go)
        if new_route:
            assert blk.levels_stored == stored_pair(L)
        return out.detach(), [t.grad for t in (f1, f2, W, b)]

    out_new, g_new = run(True)
    out_ref, g_ref = run(False)
    assert same_bits(out_new, out_ref)
    for name, x, y in zip(("df1", "df2", "dW", "db"), g_new, g_ref):
        assert x is not None and same_bits(x, y), name


def test_several_calls_on_one_block():
    """Three fused calls (fp32, fp16 and fp32 output) at different coords
    plus one plain lookup on one block: the gradients equal the all-unfused
    graph's at the project's fp32 bound, and nothing was pooled."""
    shape = SHAPES[1]
    B, D, H, W1, W2, L, r, cout = shape
    inp = inputs(shape)
    g = torch.Generator().manual_seed(7)
    shifts = [0.0, -3.25, 5.5, -8.125]
    gouts = [torch.randn(B, cout, H, W1, generator=g).to(DEV) for _ in range(3)]
    gplain = torch.randn(B, L * (2 * r + 1), H, W1, generator=g).to(DEV)

    def run(fused):
        f1 = inp["f1"].clone().requires_grad_(True)
        f2 = inp["f2"].clone().requires_grad_(True)
        W = inp["W"].clone().view(cout, -1, 1, 1).requires_grad_(True)
        b = inp["b"].clone().requires_grad_(True)
        blk = CorrBlock1D(f1, f2, num_levels=L, radius=r)
        loss = 0.0
        for s, go in zip(shifts[:3], gouts):
            c = inp["finite"] + s
            out = (blk.lookup_convc1(c, W, b, differentiable=True) if fused
                   else torch.relu(F.conv2d(blk(c), W, b)))
            loss = loss + (out * go).sum()
        loss = loss + (blk(inp["finite"] + shifts[3]) * gplain).sum()
        loss.backward()
        if fused:
            assert blk.levels_stored == [0, 2]
        return [t.grad.cpu().numpy() for t in (W, b, f1, f2)]

    got, ref = run(True), run(False)
    for name, a, b in zip(("dW", "db", "df1", "df2"), got, ref):
        e = norm_err(a, b)
        print(f"several calls {name}: {e:.2e}")
        assert e <= TOL, (name, e)


@pytest.mark.parametrize("route", ["three-levels", "low-latency", "replaced-pyramid"])
def test_routes_that_do_not_change(route):
    """A 3-level block, a low_latency block and a block with a replaced
    corr_pyramid return what the per-level kernel gives on their levels, and
    with out_dtype its cast."""
    B, D, H, W1, W2, _, r, cout = SHAPES[1]
    L = 3 if route == "three-levels" else 4
    g = torch.Generator().manual_seed(77)
    f1 = torch.randn(B, D, H, W1, generator=g).to(DEV)
    f2 = torch.randn(B, D, H, W2, generator=g).to(DEV)
    c = special_coords(B, H, W1, W2, g).to(DEV)
    W = (torch.randn(cout, L * (2 * r + 1), generator=g) / 6).to(DEV)
    b = torch.randn(cout, generator=g).to(DEV)
    with torch.no_grad():
        blk = CorrBlock1D(f1, f2, num_levels=L, radius=r, low_latency=route == "low-latency")
        if route == "replaced-pyramid":
            blk.corr_pyramid = [t.clone() for t in blk.corr_pyramid]
        a = blk.lookup_convc1(c, W, b)
        assert set(range(L)) <= set(blk.levels_stored)          # the per-level kernel's levels are in memory
        ref = rcorr.lookup_convc1(blk.corr_pyramid, c, L, r, W, b, True)
        assert a.dtype == torch.float32 and same_bits(a, ref)
        for dt in (FP16, BF16):
            h = blk.lookup_convc1(c, W, b, out_dtype=dt)
            assert h.dtype == dt and same_bits(h, ref.to(dt))


def test_network_hands_convc2_the_autocast_dtype():
    """RAFTStereo(fuse_convc1=True, corr_out_dtype="autocast") under mixed
    precision: lookup_convc1 returns the autocast dtype every iteration and
    every prediction is within the project's 0.01 px MAE of the same seeded
    network without the option."""
    from raft_stereo_amd.network import RAFTStereo, StereoArgs

    g = torch.Generator().manual_seed(8)
    img1 = (torch.rand(1, 3, 64, 96, generator=g) * 255).to(DEV)
    img2 = torch.roll(img1, -4, dims=-1)
    args = StereoArgs(mixed_precision=True)
    seen = []

    class Spy(CorrBlock1D):
        def lookup_convc1(self, *a, **kw):
            out = super().lookup_convc1(*a, **kw)
            seen.append((out.dtype, tuple(self.levels_stored)))
            return out

    def run(**kw):
        torch.manual_seed(0)
        model = RAFTStereo(args, corr_block=Spy, fuse_convc1=True, **kw).eval().to(DEV)
        del seen[:]
        with torch.no_grad():
            preds = model(img1, img2, iters=3)
        return [p.float().cpu() for p in preds], list(seen)

    base, seen_base = run()
    got, seen_opt = run(corr_out_dtype="autocast")
    assert seen_base == [(torch.float32, (0, 2))] * 3
    assert seen_opt == [(torch.float16, (0, 2))] * 3
    assert len(got) == len(base) == 3
    for i, (p, q) in enumerate(zip(got, base)):
        mae = (p - q).abs().mean().item()
        print(f"iteration {i}: MAE {mae:.3e} px")
        assert mae <= 0.01, (i, mae)
