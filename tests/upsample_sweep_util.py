"""Guarded raw C-ABI callers, references, the one-hot routing cases and the
sweep lists of the convex upsampler's sweeps (test_upsample_sweep_gpu.py,
test_upsample_sweep_host.py), on top of the arena of sweep_util.py.

Both callers carve flow, mask, grad_out and every output of one call out of
one arena (regions at 16 or 80 mod 128 between 4 KiB guards of a NaN pattern),
call the entry point through ``_lib.lib()`` with the arena's addresses and, on
return, run ``_lib.check``, ``assert_guards_intact`` (guards and inputs
bit-identical) and ``assert_outputs_written`` (no output element still the
pattern).  An over-read that reaches the arithmetic meets NaN, so with
``finite=True`` (the default) they also assert finite outputs.

A case is (N, C, H, W, f): flow (N, C, H, W), mask (N, 9 f^2, H, W).
"""
import functools

import numpy as np
import torch

import sweep_util as su
import upsample_bwd_ref
from oracle import torch_ref
from raft_stereo_amd import _lib

FACTORS = (1, 2, 4, 8)
SCALES = (2.0, 40.0)                    # mask = randn * scale; 40: a saturated softmax


# ---------------------------------------------------------------- callers

def _spec(name, t):
    return (name, t.numel() * 4, t)


def guarded_upsample(dev, flow, mask, f, phase=0, finite=True):
    """rc_convex_upsample on arena memory.  flow, mask: fp32 CPU tensors.
    Returns out (N, C, fH, fW) as a numpy array."""
    N, C, H, W = flow.shape
    assert tuple(mask.shape) == (N, 9 * f * f, H, W)
    oshape = (N, C, f * H, f * W)
    ar = su.arena(dev, [_spec("flow", flow), _spec("mask", mask), ("out", int(np.prod(oshape)) * 4, None)], phase)
    rc = _lib.lib().rc_convex_upsample(ar.ptr("flow"), ar.ptr("mask"), N, C, H, W, f, ar.ptr("out"), None)
    _lib.check(rc, "rc_convex_upsample")
    ar.assert_guards_intact()
    ar.assert_outputs_written(["out"])
    out = ar.region("out", np.float32).reshape(oshape).copy()
    if finite:
        assert np.isfinite(out).all(), "non-finite output"
    return out


def ws_floats(N, C, H, W):
    """RC_UPSAMPLE_BWD_WS of include/raftcorr.h."""
    return N * C * 9 * H * W


def guarded_upsample_backward(dev, flow, mask, gout, f, need_flow=True, need_mask=True, phase=0, finite=True):
    """rc_convex_upsample_backward on arena memory.  A gradient that is not
    requested is passed as NULL.  The workspace pointer is always passed: with
    ``need_flow`` a region of exactly RC_UPSAMPLE_BWD_WS floats that must be
    written in full (the gather reads all nine planes); without it the same
    region is registered as an input holding the pattern, which the launcher
    must leave untouched.  Returns (grad_flow, grad_mask), None where not
    requested."""
    N, C, H, W = flow.shape
    assert tuple(mask.shape) == (N, 9 * f * f, H, W) and tuple(gout.shape) == (N, C, f * H, f * W)
    nws = ws_floats(N, C, H, W)
    specs = [_spec("flow", flow), _spec("mask", mask), _spec("gout", gout)]
    outs = []
    if need_flow:
        specs += [("gflow", flow.numel() * 4, None), ("ws", nws * 4, None)]
        outs += ["gflow", "ws"]
    else:
        specs.append(("ws", nws * 4, torch.full((nws,), su.SENT32, dtype=torch.int32)))
    if need_mask:
        specs.append(("gmask", mask.numel() * 4, None))
        outs.append("gmask")
    ar = su.arena(dev, specs, phase)
    rc = _lib.lib().rc_convex_upsample_backward(
        ar.ptr("flow"), ar.ptr("mask"), ar.ptr("gout"), N, C, H, W, f,
        ar.ptr("gflow") if need_flow else None, ar.ptr("gmask") if need_mask else None, ar.ptr("ws"), None)
    _lib.check(rc, "rc_convex_upsample_backward")
    ar.assert_guards_intact()
    ar.assert_outputs_written(outs)
    gflow = ar.region("gflow", np.float32).reshape(tuple(flow.shape)).copy() if need_flow else None
    gmask = ar.region("gmask", np.float32).reshape(tuple(mask.shape)).copy() if need_mask else None
    if finite:
        assert all(np.isfinite(a).all() for a in (gflow, gmask) if a is not None), "non-finite gradient"
        assert not need_flow or np.isfinite(ar.region("ws", np.float32)).all(), "non-finite workspace"
    return gflow, gmask


# ------------------------------------------------------------- references

def ref_forward(flow, mask, f):
    """oracle.torch_ref.convex_upsample in fp64, as numpy."""
    return torch_ref.convex_upsample(flow.double(), mask.double(), f).numpy()


def ref_scale(flow, mask, f):
    """The same fp64 upsample of |flow|: sum_k wt_k |f flow_k|, the natural
    scale of the convex combination per output element."""
    return ref_forward(flow.abs(), mask, f)


def floor(flow, f):
    """An fp32 weight below 2^-126 flushes, and 9 taps x 2^-126 ~ 1e-37 of
    f max|flow| may be lost where every larger weight meets a zero."""
    return 1e-36 * f * float(flow.abs().max())


def elementwise_r(got, ref, S, fl, where=None):
    """max |got - ref| / (S + floor), over ``where`` (default everywhere)."""
    q = np.abs(np.asarray(got, np.float64) - ref) / (S + fl)
    return float(q.max() if where is None else q[where].max())


# The fp32 evaluation's own error relative to S.  A tap with d = max - mask
# has weight e^-d; its argument is rounded once (|d| 2^-24 absolute, so the
# same relative error of the weight), expf adds ~2 ulp, the 9-term sum, the
# reciprocal, the product with it, f * flow and the 9 FMAs one each: (d + 23)
# 2^-24 for that tap, and the output's relative error is a weighted mean of
# the taps'.  A weight survives in fp32 only for d < 126 ln 2 = 87.34 (below
# that the floor takes over), so r <= (87.34 + 23) 2^-24 = 6.6e-6 at any mask
# scale.  The GPU bound max(1e-5, 4 r_cpu) can therefore never exceed CAP.
R_FP32_MAX = (126 * np.log(2.0) + 23) * 2.0 ** -24
CAP = 4 * R_FP32_MAX                    # 2.63e-5


def seed_of(case, scale=0.0):
    N, C, H, W, f = case
    return ((((N * 131 + C) * 131 + H) * 131 + W) * 131 + f) * 2 + (scale > 10)


def inputs(case, scale):
    """flow = randn * 5, mask = randn * scale, grad_out = randn (fp32, CPU)."""
    N, C, H, W, f = case
    g = torch.Generator().manual_seed(seed_of(case, scale))
    flow = torch.randn(N, C, H, W, generator=g) * 5
    mask = torch.randn(N, 9 * f * f, H, W, generator=g) * scale
    gout = torch.randn(N, C, f * H, f * W, generator=g)
    return flow, mask, gout


@functools.lru_cache(maxsize=None)
def fwd_case(case, scale):
    """(flow, mask, ref, S, floor, r_cpu): the fp64 reference, its scale and
    the elementwise error of the fp32 CPU restatement; computed once."""
    flow, mask, _ = inputs(case, scale)
    f = case[4]
    ref, S, fl = ref_forward(flow, mask, f), ref_scale(flow, mask, f), floor(flow, f)
    r_cpu = elementwise_r(torch_ref.convex_upsample(flow, mask, f).numpy(), ref, S, fl)
    return flow, mask, ref, S, fl, r_cpu


@functools.lru_cache(maxsize=None)
def bwd_case(case, scale):
    """(flow, mask, gout, ref_flow, ref_mask) with the fp64 autograd gradients
    as numpy; computed once."""
    flow, mask, gout = inputs(case, scale)
    rf, rm = upsample_bwd_ref.autograd_fp64(flow, mask, gout, case[4])
    return flow, mask, gout, rf.numpy(), rm.numpy()


# ---------------------------------------------------------------- routing
# One-hot softmax: the mask is 0.0 at one tap of every sub-pixel and -200.0 at
# the other eight.  expf(-200) is 0 in fp32 (the smallest subnormal is e^-103),
# so sum = 1, inv = 1 and the weights are exactly (0, .., 1, .., 0): the
# forward is a gather and the backward a scatter, and any value that comes out
# different took a wrong route.

ROUTING_SHAPES = [(2, 2, 3, 7), (1, 1, 1, 1), (3, 1, 1, 13), (1, 2, 5, 66)]
OFF = -200.0


def routing_case(shape, seed):
    """shape = (N, C, H, W, f).  Returns a dict:
      sel (N, f, f, H, W) in 0..8, the selected tap of sub-pixel (i, j) of pixel (h, w);
      mask (N, 9 f^2, H, W) fp32; flow: arbitrary fp32 values;
      out: the expected forward of (flow, mask), fp32 (f is a power of two, so
        f * flow is exact), 0 where the selected tap lies outside the image;
      flow_int, gout_int: integer-valued fp32 in [-8, 8], so that every fp32
        sum of both backward kernels is exact (|P| <= 8 f^3 <= 4096, nine of
        them <= 36,864 < 2^24);
      out_int: the expected forward of (flow_int, mask), int64;
      gflow_int: the expected grad_flow of (flow_int, mask, gout_int), int64.
    Every expectation is an integer-index gather / scatter in numpy."""
    N, C, H, W, f = shape
    rng = np.random.default_rng(seed)
    sel = rng.integers(0, 9, (N, f, f, H, W))
    m = np.full((N, 9, f, f, H, W), OFF, np.float32)
    np.put_along_axis(m, sel[:, None], np.float32(0.0), axis=1)
    mask = m.reshape(N, 9 * f * f, H, W)
    flow = (rng.standard_normal((N, C, H, W)) * 5).astype(np.float32)
    flow_int = rng.integers(-8, 9, (N, C, H, W)).astype(np.float32)
    gout_int = rng.integers(-8, 9, (N, C, f * H, f * W)).astype(np.float32)
    n, i, j, h, w = np.meshgrid(*(np.arange(s) for s in (N, f, f, H, W)), indexing="ij")
    yy, xx = h + sel // 3 - 1, w + sel % 3 - 1              # the selected neighbour of (n, i, j, h, w)
    oy, ox = f * h + i, f * w + j                            # the output element of (n, i, j, h, w)

    def gather(fl):
        out = np.zeros((N, C, f * H, f * W), fl.dtype)
        padded = np.pad(fl, ((0, 0), (0, 0), (1, 1), (1, 1)))
        for c in range(C):
            out[n, c, oy, ox] = f * padded[n, c, yy + 1, xx + 1]
        return out

    gflow = np.zeros((N, C, H, W), np.int64)
    inside = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
    gi = gout_int.astype(np.int64)
    for c in range(C):
        np.add.at(gflow[:, c], (n[inside], yy[inside], xx[inside]), f * gi[n, c, oy, ox][inside])
    return dict(sel=sel, mask=torch.from_numpy(mask), flow=torch.from_numpy(flow), out=gather(flow),
                flow_int=torch.from_numpy(flow_int), gout_int=torch.from_numpy(gout_int),
                out_int=gather(flow_int.astype(np.int64)), gflow_int=gflow)


# ------------------------------------------------------------ sweep lists
# Per factor f, (N, C, H, W) -- the smallest shapes at which each mechanism
# can break.  Forward: one lane per (n, h, i, w), 256 per block, N H f W
# lanes.  Backward: one workgroup of f waves per 64 consecutive pixels of the
# flattened (n, h, w), N H W pixels; the gather one lane per grad_flow element.

WIDTHS = [(2, 2, 3, W) for W in range(1, 71)]       # rows wrap inside a wave; taps from the next 64-pixel block
HEIGHTS = [(2, 1, H, 5) for H in range(1, 10)]
IMAGES = [(N, 3, 1, 13) for N in range(1, 6)]       # up to five images in one 64-pixel block
CHANNELS = [(2, C, 3, 11) for C in range(1, 5)]
BWD_EDGES = [(1, 1, 1, 63), (1, 1, 1, 64), (1, 1, 1, 65)]
SINGLE = [(1, 1, 1, 1), (3, 2, 1, 1)]
WIDTH_BAND = 18


def fwd_edges(f):
    """N = C = H = 1: W f lanes = 256 (a full block), 256 + f (a second block
    with one lane per sub-row) and 512 - f (the second block f lanes short).
    N H f W is a multiple of f, so these are the residues 0, f and 256 - f;
    for f = 1 they are 0, 1 and 255."""
    return [(1, 1, 1, 256 // f), (1, 1, 1, 256 // f + 1), (1, 1, 1, 512 // f - 1)]


def misc(f):
    """Everything but the width sweep ((2, 2, 3, 11) is in it already)."""
    out = []
    for s in HEIGHTS + IMAGES + CHANNELS + BWD_EDGES + SINGLE + fwd_edges(f):
        if s not in WIDTHS and s not in out:
            out.append(s)
    return out


def bands(f):
    """{band name: [(N, C, H, W, f), ..]} of one factor."""
    out = {f"W{b[0][3]}-{b[-1][3]}": b for b in su.bands(WIDTHS, WIDTH_BAND)}
    out["misc"] = misc(f)
    return {k: [s + (f,) for s in v] for k, v in out.items()}


BANDS = [(f, name) for f in FACTORS for name in bands(1)]
BAND_IDS = [f"f{f}-{name}" for f, name in BANDS]


def cases(f):
    """Every case of factor f; forward and backward sweep the same list."""
    return [c for b in bands(f).values() for c in b]


def totals(case):
    """(total_fwd, total_bwd): lanes of the forward kernel, pixels of the backward."""
    N, C, H, W, f = case
    return N * H * f * W, N * H * W


PHASE_CASES = [(2, 2, 3, 23, f) for f in FACTORS]
NONFINITE_CASES = [(2, 2, 3, 9, f) for f in FACTORS]


def nonfinite_mask(case):
    """mask = randn * 2 with, per sub-pixel (n, i, j, h, w) chosen at random:
    1/4 with one to eight taps at -inf (finite output), 1/16 each with all
    nine taps -inf, one tap +inf, one tap NaN (NaN output)."""
    N, C, H, W, f = case
    flow, mask, _ = inputs(case, 2.0)
    rng = np.random.default_rng(seed_of(case))
    m = mask.numpy().reshape(N, 9, f, f, H, W).copy()
    kind = rng.integers(0, 16, (N, f, f, H, W))
    taps = rng.permuted(np.broadcast_to(np.arange(9).reshape(9, 1, 1, 1, 1, 1), (9,) + kind.shape).copy(), axis=0)
    rank = np.moveaxis(taps, 0, 1)                           # (N, 9, f, f, H, W): a permutation of 0..8 per sub-pixel
    cut = rng.integers(1, 9, kind.shape)                     # how many taps go to -inf
    m[(kind < 4)[:, None] & (rank < cut[:, None])] = -np.inf
    m[np.broadcast_to((kind == 4)[:, None], m.shape)] = -np.inf
    m[(kind == 5)[:, None] & (rank == 0)] = np.inf
    m[(kind == 6)[:, None] & (rank == 0)] = np.nan
    return flow, torch.from_numpy(m.reshape(N, 9 * f * f, H, W)), kind
