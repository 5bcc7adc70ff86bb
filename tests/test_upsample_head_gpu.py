"""rc_upsample_head on the guarded arena of sweep_util.py, through the raw C
ABI: every case of upsample_head_util at f = 1, 2, 4, 8, in fp32, fp16 and
bf16 and in both layout classes, the arena's two phases alternating.  After
every call the guards and the inputs are bit-identical and no output element
still holds the pattern (upsample_head_util.guarded_head).

Bit equality: against rc_convex_upsample on the fp32 NCHW-contiguous mask
``scale * mask.float()`` (computed on the host: one IEEE multiply, as in the
kernel), for scale 0.25 on mask = randn * 2 and scale 1.0 on mask = randn * 40.
The fp64 bound: r <= max(1e-5, 4 r_cpu) against oracle.torch_ref's upsampler
on the same widened, scaled mask, the bound of test_upsample_sweep_gpu.py, so
that the check is not only one kernel against another.
"""
import numpy as np
import pytest
import torch

import graph_util
import upsample_head_util as hu
import upsample_sweep_util as uu
from raft_stereo_amd.upsample import convex_upsample, upsample_head

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
COMBOS = ((2.0, 0.25), (40.0, 1.0))          # (mask = randn * this, the kernel's scale)


def check(case, dt, cls, mscale, scale, phase, base_off=0):
    f = case[4]
    flow, mask = hu.case_inputs(case, mscale, dt)
    got = hu.guarded_head(DEV, flow, mask, f, dt, cls, scale, phase=phase, base_off=base_off)
    want = uu.guarded_upsample(DEV, flow, (scale * mask.float()).contiguous(), f, phase=phase)
    diff = int((hu.bits(got) != hu.bits(want)).sum())
    assert not diff, f"{case} {dt} {cls} scale {scale}: {diff} of {got.size} elements differ from rc_convex_upsample"
    ref, S, fl, r_cpu = hu.reference(case, mscale, dt, scale)
    r = uu.elementwise_r(got, ref, S, fl)
    assert r <= max(1e-5, 4 * r_cpu), (case, dt, cls, mscale, scale, r, r_cpu)
    return r


@pytest.mark.parametrize("dt", sorted(hu.DTYPES))
@pytest.mark.parametrize("f", hu.FACTORS)
def test_cases(f, dt):
    worst, k = 0.0, 0
    for case in hu.cases(f):
        for cls in hu.CLASSES:
            for mscale, scale in COMBOS:
                worst = max(worst, check(case, dt, cls, mscale, scale, phase=k % 2))
                k += 1
    print(f"f = {f}, {dt}: {k} calls bit-equal to rc_convex_upsample, worst r {worst:.2e}")


@pytest.mark.parametrize("dt", sorted(hu.DTYPES))
@pytest.mark.parametrize("f", hu.FACTORS)
def test_narrow_fallback(f, dt):
    """(1, 1, 2, 5) at the arena's odd phase with the mask's base one element
    past its region's start: neither 8 bytes (planar) nor f elements
    (interleaved, f > 1) divide it, so the host picks the one-element loads."""
    case = hu.ODD + (f,)
    for cls in hu.CLASSES:
        assert not hu.wide(case, dt, cls, hu.es(dt)) or (cls == "interleaved" and f == 1)
        for mscale, scale in COMBOS:
            check(case, dt, cls, mscale, scale, phase=1, base_off=hu.es(dt))


@pytest.mark.parametrize("dt", sorted(hu.DTYPES))
@pytest.mark.parametrize("f", hu.FACTORS)
def test_one_hot_routing_interleaved(f, dt):
    """Logit 0 at one tap and -200 at the other eight (exact in bf16 and
    fp16): the output is a gather, compared with numpy's integer indexing.
    Pins the channel index k f^2 + i f + j under channel stride 1."""
    for s, shape in enumerate(uu.ROUTING_SHAPES):
        rc = uu.routing_case(shape + (f,), 100 * f + s)
        mask = rc["mask"].to(hu.DTYPES[dt])
        assert torch.equal(mask.float(), rc["mask"])
        for cls in hu.CLASSES:
            got = hu.guarded_head(DEV, rc["flow"], mask, f, dt, cls, 1.0, phase=s % 2)
            assert np.array_equal(got, rc["out"]), (shape, f, dt, cls)


@pytest.mark.parametrize("cls", hu.CLASSES)
@pytest.mark.parametrize("f", hu.FACTORS)
def test_flow_as_a_channel_slice(f, cls):
    """The first C channels of an (N, C + 1, H, W) tensor, passed by strides,
    give the contiguous copy's bits (the other channel holds NaN)."""
    for case in ((2, 1, 3, 21, f), (2, 2, 3, 22, f)):
        flow, mask = hu.case_inputs(case, 2.0, "bf16")
        a = hu.guarded_head(DEV, flow, mask, f, "bf16", cls, 0.25, flow_slice=True)
        b = hu.guarded_head(DEV, flow, mask, f, "bf16", cls, 0.25)
        assert np.array_equal(hu.bits(a), hu.bits(b))


@pytest.mark.parametrize("dt", sorted(hu.DTYPES))
@pytest.mark.parametrize("f", hu.FACTORS)
def test_nonfinite_logits(f, dt):
    """-inf, +inf and NaN logits: NaN exactly where the fp64 reference has it,
    the bound everywhere else."""
    case = (2, 2, 3, 9, f)
    flow, mask32, kind = uu.nonfinite_mask(case)
    mask = mask32.to(hu.DTYPES[dt])
    m32 = 0.25 * mask.float()
    ref, S, fl = uu.ref_forward(flow, m32, f), uu.ref_scale(flow, m32, f), uu.floor(flow, f)
    assert np.isnan(ref).any() and not np.isnan(ref).all()
    for p, cls in enumerate(hu.CLASSES):
        got = hu.guarded_head(DEV, flow, mask, f, dt, cls, 0.25, phase=p, finite=False)
        assert np.array_equal(np.isnan(got), np.isnan(ref)), (f, dt, cls)
        ok = ~np.isnan(ref)
        assert np.isfinite(got[ok]).all()
        r_cpu = uu.elementwise_r(uu.torch_ref.convex_upsample(flow, m32, f).numpy(), ref, S, fl, ok)
        assert uu.elementwise_r(got, ref, S, fl, ok) <= max(1e-5, 4 * r_cpu)


def _dense_variants(mask):
    """The mask NCHW-dense, channels-last-dense, as a batch slice of each, and
    in a layout of neither class."""
    MC = mask.shape[1]
    cl = torch.channels_last
    wide = torch.cat([mask, mask], 1)
    yield "nchw", mask.contiguous()
    yield "channels_last", mask.contiguous(memory_format=cl)
    yield "nchw_channel_slice", wide[:, :MC]                                          # planar, a larger batch stride
    yield "channels_last_batch_step", torch.repeat_interleave(mask, 2, 0).contiguous(memory_format=cl)[::2]
    yield "channels_last_channel_slice", wide.contiguous(memory_format=cl)[:, :MC]    # neither class: copied
    yield "transposed", mask.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2)     # neither class: copied


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16], ids=["f32", "f16", "bf16"])
def test_python_wrapper_against_the_composed_route(dtype):
    """upsample.upsample_head on tensors as the network hands them over --
    the x-slice of an (N, 2, h, w) flow, the mask in every layout -- equals
    convex_upsample(flow, 0.25 * mask.float()) bit for bit."""
    g = torch.Generator().manual_seed(5)
    flow2 = (torch.randn(2, 2, 7, 12, generator=g) * 5).to(DEV)
    mask = (torch.randn(2, 144, 7, 12, generator=g) * 2).to(dtype).to(DEV)
    want = convex_upsample(flow2[:, :1], 0.25 * mask.float(), 4)
    for name, m in _dense_variants(mask):
        got = upsample_head(flow2[:, :1], m, 4)
        assert got.dtype == torch.float32 and got.is_contiguous()
        assert torch.equal(graph_util.bits(got), graph_util.bits(want)), name
    assert tuple(upsample_head(flow2[:0, :1], mask[:0], 4).shape) == (0, 1, 28, 48)


def test_graph_capture_bf16_interleaved():
    """(2, 1, 7, 9), f = 4, a bf16 channels-last mask: captured, replayed,
    refilled and replayed again with the eager call's bits (graph_util)."""
    def inputs(seed):
        g = torch.Generator().manual_seed(seed)
        flow = torch.randn(2, 1, 7, 9, generator=g) * 5
        mask = (torch.randn(2, 144, 7, 9, generator=g) * 8).bfloat16().contiguous(memory_format=torch.channels_last)
        return [flow, mask]

    def fn(flow, mask):
        assert mask.stride(1) == 1
        return upsample_head(flow, mask, 4, 0.25)

    graph_util.captured(fn, inputs(1), inputs(2))
