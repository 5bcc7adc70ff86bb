"""Every entry point under graph capture and replay ("Graph
capture"): each scenario goes through graph_util.captured -- eager on fresh
tensors, captured, replayed after the static inputs were refilled in place --
and every comparison is bit equality with the eager run of the same wrapper.

Shapes are rows of the existing test file of each family (cited where they
are bound to a name).  For the lookups it is the smallest row on which the
protocol's discrimination condition can hold: special_coords draws x from
[w1 - 64, w1], so on the 20-pixel rows ((1, 8, 2, 20, 16, 4, 1) and its
like) most taps of most pixels fall left of the image and are zero whatever
the fmaps hold -- the reference's own output differs between two seeds in
0.39 of its elements there, in 0.59 .. 0.79 on the rows used here.
"""
import types

import pytest
import torch

from graph_util import DEV, bits, captured, same_bits
from raft_stereo_amd import CorrBlock1D, corr, gru, upsample
from raft_stereo_amd.network import ConvGRU
from test_corr_gpu import special_coords

pytestmark = pytest.mark.gpu
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
SEED_A, SEED_B = 101, 202

# B, D, H, W1, W2, L, r
PAIR4 = (1, 16, 3, 45, 45, 4, 3)        # test_corr_gpu.py CHAIN_SHAPES and BF16_PAIR_SHAPES: 4 levels, the pair kernel
PAIR2 = (1, 16, 2, 50, 50, 2, 4)        # test_corr_gpu.py BF16_PAIR_SHAPES: 2 levels
CHAIN3 = (1, 16, 2, 60, 61, 3, 4)       # test_corr_gpu.py CHAIN_SHAPES: 3 levels, the level-1 chain kernel
RECORDS = (1, 256, 3, 100, 100, 4, 4)   # test_records_gpu.py SHAPES, its smallest row
SHEARED = (2, 16, 3, 48, 96, 2, 2)      # test_disparity_gpu.py SHAPES, its smallest row
CONVC1 = (1, 8, 1, 20, 16, 4, 1, 8)     # test_pair_convc1_gpu.py / test_convc1_backward_gpu.py SHAPES[0] (.., cout)
CONVC1_3 = (3, 8, 2, 130, 129, 3, 3, 63)  # test_convc1_backward_gpu.py SHAPES: its only 3-level row (per-level route)
BUILD_BWD = (1, 8, 3, 36, 40)           # test_backward_split_gpu.py SHAPES, the "tiny" pair4 row
UPSAMPLE = {4: (2, 2, 7, 9, 4), 8: (1, 2, 5, 5, 8)}   # test_upsample.py SHAPES (N, C, H, W, factor)
GRU = (1, 8, 3, 3, 5)                   # test_gru_gates_gpu.py SHAPES[0]: N, C, Cx, H, W
# test_gru_inputs_gpu.py CASES: (N, H, W), ((mode, C, h, w), ...)
ASSEMBLE = {"tiny": ((1, 3, 5), (("copy", 8, 3, 5), ("pool", 3, 5, 9), ("bilinear", 5, 2, 3))),
            "w6": ((1, 2, 6), (("copy", 2, 2, 6), ("pool", 2, 3, 11), ("bilinear", 2, 2, 2)))}


@pytest.fixture(autouse=True)
def inference():
    with torch.no_grad():
        yield


@pytest.fixture
def pinned_convs(monkeypatch):
    """Deterministic convolution algorithms, as test_gru_inputs_network_gpu.py asks for them."""
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    monkeypatch.setattr(torch.backends.cudnn, "benchmark", False)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def fmaps(shape, g, dt=F32):
    B, D, H, W1, W2 = shape[:5]
    return [torch.randn(B, D, H, W1, generator=g).to(dt), torch.randn(B, D, H, W2, generator=g).to(dt)]


def coords(shape, g, n=1):
    B, D, H, W1, W2 = shape[:5]
    return [special_coords(B, H, W1, W2, g) for _ in range(n)]


def finite_coords(shape, g):
    """special_coords with its NaN and +-inf entries replaced by a finite x
    left of the image, for the fused-conv backward: there one NaN correlation
    row makes every element of the weight gradient NaN (0 * NaN in the sum
    over the pixels, as in PyTorch's), on A and on B alike."""
    c = coords(shape, g)[0]
    c[~torch.isfinite(c)] = -7.25
    return [c]


def grad_outs(shape, g, n=1):
    B, D, H, W1, W2, L, r = shape[:7]
    return [torch.randn(B, L * (2 * r + 1), H, W1, generator=g) for _ in range(n)]


def conv_params(shape, g):
    L, r, cout = shape[5:8]
    cin = L * (2 * r + 1)
    return [torch.randn(cout, cin, 1, 1, generator=g) * cin ** -0.5, torch.randn(cout, generator=g)]


def both(make):
    """The scenario's inputs drawn from the two seeds."""
    return make(gen(SEED_A)), make(gen(SEED_B))


# ---------------------------------------------------------------- build + lookups

BUILD = {
    "fp32_split": (PAIR4, F32, {}),
    "exact_f32": (PAIR4, F32, {"exact_f32": True}),
    "bf16_fmaps": (PAIR4, BF16, {}),
    "bf16_pyramid": (PAIR4, F32, {"pyramid_dtype": BF16}),
    "f16_pyramid": (PAIR4, F32, {"pyramid_dtype": F16}),
    "levels2": (PAIR2, F32, {}),
    "levels3": (CHAIN3, F32, {}),
    "levels4": (PAIR4, F32, {"shadow": False}),
    "shadow": (PAIR4, F32, {"shadow": True}),
    "channels_last": (PAIR4, F32, {"channels_last": True}),
    "out_f16": (PAIR4, F32, {"out_dtype": F16}),
    "out_bf16": (PAIR4, F32, {"out_dtype": BF16}),
    "low_latency": (PAIR4, F32, {"low_latency": True}),
    "disparity": (SHEARED, F32, {"layout": "disparity"}),
    "records": (RECORDS, F32, {"layout": "records"}),
}


@pytest.mark.parametrize("name", sorted(BUILD))
def test_build_and_three_lookups(name):
    """The block is constructed inside the capture (the pyramid comes from
    the graph's pool), then looked up three times."""
    shape, dt, kw = BUILD[name]
    L, r = shape[5:7]

    def fn(f1, f2, *cs):
        blk = CorrBlock1D(f1, f2, num_levels=L, radius=r, **kw)
        return [blk(c) for c in cs]

    a, b = both(lambda g: fmaps(shape, g, dt) + coords(shape, g, 3))
    captured(fn, a, b)


# ---------------------------------------------------------------- a block built outside

def outside_block(shape, **kw):
    """A factory of blocks on fixed fmaps, built eagerly."""
    f1, f2 = (t.to(DEV) for t in fmaps(shape, gen(7)))
    L, r = shape[5:7]
    return lambda: CorrBlock1D(f1, f2, num_levels=L, radius=r, **kw)


def outside_scenario(kind):
    """(factory of fn, inputs A, inputs B)."""
    if kind == "call":
        new = outside_block(PAIR4)
        return (lambda: new().__call__), *both(lambda g: coords(PAIR4, g))
    if kind == "lookup_step":
        new = outside_block(PAIR4)
        return (lambda: new().lookup_step), *both(lambda g: coords(PAIR4, g) + [torch.randn(1, 2, 3, 45, generator=g)])
    if kind == "convc1_pair":
        new = outside_block(CONVC1)
        return (lambda: new().lookup_convc1), *both(lambda g: coords(CONVC1, g) + conv_params(CONVC1, g))
    if kind == "convc1_levels":          # 3 levels: the per-level kernel on levels pooled on first use
        new = outside_block(CONVC1_3)
        return (lambda: new().lookup_convc1), *both(lambda g: coords(CONVC1_3, g) + conv_params(CONVC1_3, g))
    assert kind == "corr_pyramid"        # read for the first time inside fn: levels 1 and 3 are pooled there
    new = outside_block(PAIR4)

    def make():
        blk = new()
        assert blk.levels_stored == [0, 2]
        return lambda c: corr.lookup(blk.corr_pyramid, c, 4, 3)

    return make, *both(lambda g: coords(PAIR4, g))


@pytest.mark.parametrize("cold", [False, True], ids=["warm", "cold"])
@pytest.mark.parametrize("kind", ["call", "lookup_step", "convc1_pair", "convc1_levels", "corr_pyramid"])
def test_lookups_on_a_block_built_outside(kind, cold):
    make, a, b = outside_scenario(kind)
    captured(None, a, b, cold=cold, make=make)


# ---------------------------------------------------------------- raw wrappers

def test_raw_lookup():
    L, r = PAIR4[5:7]
    captured(lambda f1, f2, c: corr.lookup(corr.build_pyramid(f1, f2, L), c, L, r),
             *both(lambda g: fmaps(PAIR4, g) + coords(PAIR4, g)))


def test_raw_pool_level():
    P, W = PAIR4[2] * PAIR4[3], PAIR4[4]
    captured(corr.pool_level, *both(lambda g: [torch.randn(P, 1, 1, W, generator=g)]))


def test_raw_lookup_records():
    r, W2 = RECORDS[6], RECORDS[4]
    captured(lambda f1, f2, c: corr.lookup_records(corr.build_records(f1, f2), c, r, W2),
             *both(lambda g: fmaps(RECORDS, g) + coords(RECORDS, g)))


# ---------------------------------------------------------------- backward wrappers
# Called directly.  The level-gradient buffers are zeroed inside fn, so every
# replay starts from the same state.  A level gradient holds at most 2r + 2
# entries per pixel row: the fmap gradients folded from them by build_backward
# are the dense outputs the discrimination condition is judged on; the level
# gradients themselves are compared bit for bit like every output.

def level_grads(shape, zero=True):
    B, D, H, W1, W2, L, r = shape[:7]
    return corr.grad_buffers(B * H * W1, [W2 >> l for l in range(L)], torch.device(DEV), pair=True, zero=zero)


def test_lookup_backward():
    L, r = PAIR4[5:7]

    def fn(c, go, f1, f2):
        grads = level_grads(PAIR4)
        corr.lookup_backward(grads, c, go, L, r)
        return [*corr.build_backward(f1, f2, grads), *grads]

    captured(fn, *both(lambda g: coords(PAIR4, g) + grad_outs(PAIR4, g) + fmaps(PAIR4, g)), judged=[0, 1])


@pytest.mark.parametrize("overwrite", [False, True], ids=["add", "overwrite"])
def test_lookup_backward_calls(overwrite):
    L, r = PAIR4[5:7]

    def fn(c0, c1, c2, g0, g1, g2, f1, f2):
        grads = level_grads(PAIR4, zero=not overwrite)
        corr.lookup_backward_calls(grads, [c0, c1, c2], [g0, g1, g2], L, r, overwrite=overwrite)
        return [*corr.build_backward(f1, f2, grads), *grads]

    captured(fn, *both(lambda g: coords(PAIR4, g, 3) + grad_outs(PAIR4, g, 3) + fmaps(PAIR4, g)), judged=[0, 1])


@pytest.mark.parametrize("exact", [False, True], ids=["split", "exact"])
def test_build_backward_pair_fold(exact):
    B, D, H, W1, W2 = BUILD_BWD
    P = B * H * W1

    def fn(f1, f2, v0, v2):
        grads = level_grads(BUILD_BWD + (4, 4))
        grads[0].copy_(v0)
        grads[2].copy_(v2)
        return corr.build_backward(f1, f2, grads, exact_f32=exact)

    captured(fn, *both(lambda g: fmaps(BUILD_BWD, g) + [torch.randn(P, W2, generator=g),
                                                       torch.randn(P, W2 >> 2, generator=g)]))


@pytest.mark.parametrize("chain", [False, True], ids=["levels", "pair"])
def test_convc1_backward(chain):
    """Both fused-conv backward entry points (each zeroes its weight and bias
    sums with a memset node on the stream)."""
    L, r = CONVC1[5:7]

    def fn(f1, f2, c, w, b, go):
        if chain:
            pyr = corr.build_pyramid(f1, f2, 3, skip=(1,))
            return corr.lookup_chain_convc1_backward(pyr, c, L, r, w, b, True, go)
        return corr.lookup_convc1_backward(corr.build_pyramid(f1, f2, L), c, L, r, w, b, True, go)

    B, D, H, W1 = CONVC1[:4]
    captured(fn, *both(lambda g: fmaps(CONVC1, g) + finite_coords(CONVC1, g) + conv_params(CONVC1, g) +
                       [torch.randn(B, CONVC1[7], H, W1, generator=g)]))


def upsample_backward(flow, mask, gout, factor):
    """rc_convex_upsample_backward as the autograd node calls it."""
    ctx = types.SimpleNamespace(saved_tensors=(flow, mask), needs_input_grad=(True, True, False), factor=factor,
                                dtypes=(flow.dtype, mask.dtype))
    return upsample._ConvexUpsample.backward(ctx, gout)[:2]


def upsample_inputs(shape, g):
    N, C, H, W, f = shape
    return [torch.randn(N, C, H, W, generator=g), torch.randn(N, 9 * f * f, H, W, generator=g)]


def test_upsample_backward():
    N, C, H, W, f = UPSAMPLE[4]
    captured(lambda fl, m, go: upsample_backward(fl, m, go, f),
             *both(lambda g: upsample_inputs(UPSAMPLE[4], g) + [torch.randn(N, C, f * H, f * W, generator=g)]))


# ---------------------------------------------------------------- upsampler

@pytest.mark.parametrize("factor", [4, 8])
def test_convex_upsample(factor):
    shape = UPSAMPLE[factor]
    captured(lambda fl, m: upsample.convex_upsample(fl, m, factor), *both(lambda g: upsample_inputs(shape, g)))


# ---------------------------------------------------------------- GRU glue

GRU_DT = {"fp32": F32, "bf16": BF16}
FORMATS = {"planar": torch.contiguous_format, "channels_last": torch.channels_last}


def gru_operands(g, n, dt, fmt, shape=None):
    N, C, Cx, H, W = GRU
    return [torch.randn(shape or (N, C, H, W), generator=g).to(dt).contiguous(memory_format=fmt) for _ in range(n)]


def gates_inplace(z_pre, r_pre, cz, cr, h):
    z = z_pre.clone()
    return gru.gru_gates(z, r_pre, cz, cr, h, z_out=z)


def blend_inplace(z, q_pre, cq, h):
    out = h.clone()
    return gru.gru_blend(z, q_pre, cq, out, h_out=out)


def gates_backward_inplace(g_z, g_rh, z, r_pre, cr, h):
    g = g_z.clone()
    return gru.gru_gates_backward(g, g_rh, z, r_pre, cr, h, g_zpre=g)


def blend_backward_inplace(g_out, z, q_pre, cq, h):
    g = g_out.clone()
    return gru.gru_blend_backward(g, z, q_pre, cq, h, g_h=g)


GLUE = {"gates": (gru.gru_gates, 5), "gates_inplace": (gates_inplace, 5),
        "blend": (gru.gru_blend, 4), "blend_inplace": (blend_inplace, 4),
        "gates_backward": (gru.gru_gates_backward, 6), "gates_backward_inplace": (gates_backward_inplace, 6),
        "blend_backward": (gru.gru_blend_backward, 5), "blend_backward_inplace": (blend_backward_inplace, 5)}


@pytest.mark.parametrize("fmt", sorted(FORMATS))
@pytest.mark.parametrize("dt", sorted(GRU_DT))
@pytest.mark.parametrize("op", sorted(GLUE))
def test_gru_glue(op, dt, fmt):
    fn, n = GLUE[op]
    captured(fn, *both(lambda g: gru_operands(g, n, GRU_DT[dt], FORMATS[fmt])))


@pytest.mark.parametrize("fmt", sorted(FORMATS))
@pytest.mark.parametrize("dt", sorted(GRU_DT))
@pytest.mark.parametrize("case", sorted(ASSEMBLE))
def test_gru_assemble(case, dt, fmt):
    (N, H, W), parts = ASSEMBLE[case]
    dtype, mf = GRU_DT[dt], FORMATS[fmt]

    def fn(*srcs):
        wrap = {"copy": lambda t: t, "pool": gru.Pooled, "bilinear": lambda t: gru.Resized(t, (H, W))}
        return gru.assemble([wrap[p[0]](t) for p, t in zip(parts, srcs)], dtype, mf)

    captured(fn, *both(lambda g: [torch.randn(N, C, h, w, generator=g).to(dtype).contiguous(memory_format=mf)
                                  for _, C, h, w in parts]))


@pytest.mark.parametrize("cold", [False, True], ids=["warm", "cold"])
@pytest.mark.parametrize("fmt", sorted(FORMATS))
@pytest.mark.parametrize("dt", sorted(GRU_DT))
def test_conv_gru_forward(dt, fmt, cold, pinned_convs):
    """One ConvGRU through gru.conv_gru_forward: the stacked gate weights of
    gru._ZR are made by the warm-up call, or (cold) inside the capture."""
    N, C, Cx, H, W = GRU
    dtype, mf = GRU_DT[dt], FORMATS[fmt]

    def make():
        torch.manual_seed(3)
        m = ConvGRU(C, Cx).eval().to(DEV).to(dtype).to(memory_format=mf)
        return lambda h, cz, cr, cq, x: gru.conv_gru_forward(m, h, cz, cr, cq, x)

    def inputs(g):
        h, cz, cr, cq = gru_operands(g, 4, dtype, mf)
        return [torch.tanh(h.float()).to(dtype), cz, cr, cq, *gru_operands(g, 1, dtype, mf, (N, Cx, H, W))]

    captured(None, *both(inputs), cold=cold, make=make)


# ---------------------------------------------------------------- non-contiguous inputs
# The wrappers copy such operands (.contiguous(), .float()).  The copy has to
# be a node of the graph that re-reads the caller's buffer on every replay;
# a copy made once at capture time would answer the refill with A's result.

def wide(t, g):
    """``t`` as columns 1 .. W of a tensor three columns wider: (the wide tensor's values)."""
    w = torch.randn(*t.shape[:-1], t.shape[-1] + 3, generator=g)
    w[..., 1:t.shape[-1] + 1] = t
    return w


def narrow(w):
    return w[..., 1:w.shape[-1] - 2]


def test_noncontiguous_coords_and_bf16_delta():
    """coords as a column slice of a wider tensor (its rows are W1 + 3 apart:
    _check_coords and lookup_step copy it), delta in bf16 (lookup_step widens
    it), through the block's call and its lookup_step."""
    blk = outside_block(PAIR4)()

    def fn(cw, d):
        c = narrow(cw)
        assert not c.is_contiguous() and d.dtype == BF16
        return [blk(c), *blk.lookup_step(c, d)]

    captured(fn, *both(lambda g: [wide(coords(PAIR4, g)[0], g), torch.randn(1, 2, 3, 45, generator=g).to(BF16)]))


def test_permuted_fmaps():
    """fmaps as permuted views of (B, H, W, D) tensors: the build copies them."""
    L, r = PAIR4[5:7]

    def fn(f1, f2, c):
        f1, f2 = f1.permute(0, 3, 1, 2), f2.permute(0, 3, 1, 2)
        assert not f1.is_contiguous()
        return CorrBlock1D(f1, f2, num_levels=L, radius=r)(c)

    captured(fn, *both(lambda g: [f.permute(0, 2, 3, 1).contiguous() for f in fmaps(PAIR4, g)] + coords(PAIR4, g)))


def test_noncontiguous_grad_out_and_weight():
    """grad_out as a column slice (lookup_backward, the fused-conv backward)
    and convc1's weight as a transposed view."""
    L, r, cout = CONVC1[5:8]
    B, D, H, W1 = CONVC1[:4]

    def fn(f1, f2, c, wt, b, gow, gcw):
        w, go, gc = wt.t()[:, :, None, None], narrow(gow), narrow(gcw)
        assert not (w.is_contiguous() or go.is_contiguous() or gc.is_contiguous())
        grads = level_grads(CONVC1)
        corr.lookup_backward(grads, c, gc, L, r)
        pyr = corr.build_pyramid(f1, f2, L)
        return [*corr.lookup_convc1_backward(pyr, c, L, r, w, b, True, go), *corr.build_backward(f1, f2, grads),
                *grads]

    def inputs(g):
        w, b = conv_params(CONVC1, g)
        return (fmaps(CONVC1, g) + finite_coords(CONVC1, g) + [w[:, :, 0, 0].t().contiguous(), b] +
                [wide(torch.randn(B, cout, H, W1, generator=g), g), wide(grad_outs(CONVC1, g)[0], g)])

    captured(fn, *both(inputs), judged=[0, 1, 2, 3, 4])


# ---------------------------------------------------------------- what a capture refuses, what it may not change

def test_check_finite_raises_before_any_launch():
    """check_finite=True reads a reduction's result on the host: inside a
    capture it raises before anything is launched, and leaves the library
    usable -- an eager block afterwards gives the bits it gave before."""
    L, r = PAIR4[5:7]
    f1, f2, c = (t.to(DEV) for t in fmaps(PAIR4, gen(SEED_A)) + coords(PAIR4, gen(SEED_A)))
    before = bits(CorrBlock1D(f1, f2, num_levels=L, radius=r, check_finite=True)(c))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    # torch warns when a capture ends with no node in it: nothing was launched
    with pytest.warns(UserWarning, match="Graph is empty"):
        with pytest.raises(RuntimeError, match="check_finite=True inside a graph capture"):
            with torch.cuda.graph(graph):
                CorrBlock1D(f1, f2, num_levels=L, radius=r, check_finite=True)
    assert not torch.cuda.is_current_stream_capturing()
    after = bits(CorrBlock1D(f1, f2, num_levels=L, radius=r, check_finite=True)(c))
    torch.cuda.synchronize()
    same_bits([after], [before], "eager block after the refused capture")


def test_auto_layout_is_the_same_inside_a_capture():
    """layout="auto" is decided from shapes, dtypes and options alone."""
    L, r = RECORDS[5:7]
    seen = []

    def fn(f1, f2, c):
        blk = CorrBlock1D(f1, f2, num_levels=L, radius=r, layout="auto")
        seen.append((blk.layout, torch.cuda.is_current_stream_capturing()))
        return blk(c)

    captured(fn, *both(lambda g: fmaps(RECORDS, g, BF16) + coords(RECORDS, g)))
    assert {cap for _, cap in seen} == {False, True}
    assert len({layout for layout, _ in seen}) == 1, seen
    f1, f2 = (t.to(DEV) for t in fmaps(RECORDS, gen(1), BF16))
    assert seen[0][0] == corr.auto_layout(f1, f2, L, r)
