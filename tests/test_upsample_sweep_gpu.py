"""The convex upsampler's three kernels (csrc/upsample.hip) through the raw C
ABI on guarded memory: convex_upsample_kernel<F>, convex_upsample_bwd_kernel<F>
and convex_upsample_bwd_gather_kernel, F = 1, 2, 4, 8.

Every call goes through upsample_sweep_util.guarded_upsample /
guarded_upsample_backward: flow, mask, grad_out and the outputs lie in one
arena (sweep_util.py) at addresses 16 or 80 mod 128 between 4 KiB guards of a
NaN pattern, the phase alternating from case to case.  After the call the
guards and the inputs must be bit-identical, no output element may still hold
the pattern -- the backward's workspace included, all nine planes of which the
gather reads -- and every output must be finite.  A gradient that is not
requested is NULL; without grad_flow the workspace region is an input holding
the pattern, which the launcher must leave alone.

Shapes (N, C, H, W), each at every F (upsample_sweep_util.py;
test_upsample_sweep_host.py asserts the claims from the lists):
  (2, 2, 3, W), W = 1..70   rows that wrap inside a wave, taps that belong to
                            the neighbouring 64-pixel workgroup, 1..7 workgroups;
  (2, 1, H, 5), H = 1..9;   (N, 3, 1, 13), N = 1..5: up to five images in one
  64-pixel workgroup;       (2, C, 3, 11), C = 1..4;
  (1, 1, 1, W), W = 63, 64, 65: N H W = 63, 0, 1 mod 64 (the backward's
  workgroup); W = 256/F, 256/F + 1, 512/F - 1: N H F W = 0, F, 256 - F mod 256
  (the forward's block; the lane count is a multiple of F);
  (1, 1, 1, 1) and (3, 2, 1, 1): every neighbour outside the image.

Bounds:
  forward, elementwise: r = max |got - ref| / (S + floor) against
    oracle.torch_ref.convex_upsample in fp64, S the same fp64 upsample of
    |flow| (the scale of each element's convex combination, so an error in a
    region of small flow is not divided by the largest flow elsewhere), floor
    = 1e-36 f max|flow| (fp32 weights below 2^-126 flush).  r <= max(1e-5,
    4 x r of the fp32 CPU restatement on the same inputs), the rule of
    test_upsample_backward_gpu.test_saturated_softmax; 4 r_cpu <= 2.63e-5 on
    every input (upsample_sweep_util.CAP, test_upsample_sweep_host.py).
    Inputs: flow = randn * 5 with mask = randn * 2 and with mask = randn * 40.
  backward: golden_util.norm_err against fp64 autograd per gradient, <= 1e-5
    at scale 2 and <= max(1e-5, 4 x upsample_bwd_ref.restated_backward in
    fp32) at scale 40, the bounds of test_upsample_backward_gpu.py.  The
    flow-only and mask-only calls are bit-equal to the call with both.
  routing: a mask of 0 at one tap and -200 at the other eight makes the
    weights exactly one-hot, so the forward is a gather (arbitrary fp32 flow;
    f * flow is exact) and grad_flow an integer scatter (flow and grad_out
    integers in [-8, 8]: every fp32 sum is exact); both are compared with
    np.array_equal against numpy integer indexing, grad_mask against 0.  This
    pins the tap order k = 3 (dy + 1) + (dx + 1), the sub-pixel channel
    k f^2 + i f + j and the mirrored taps of the gather.
  non-finite masks: NaN in exactly the elements where the fp64 reference has
    NaN, the forward bound on the others.

Measured on one MI355X (the largest value any band printed):
  forward r: 4.96e-7 at scale 2 (bound 1e-5), 3.98e-6 at scale 40 (bound
    1.59e-5; the fp32 CPU restatement: 5.16e-7 and 3.99e-6);
  backward norm_err at scale 2: grad_flow 2.86e-7, grad_mask 6.60e-7; at
    scale 40: grad_flow 2.16e-7, grad_mask 4.68e-6 -- except on four shapes of
    at most 20 pixels at f <= 2, (1, 1, 1, 1), (2, 1, 1, 5), (2, 1, 2, 5) at
    f = 1 and (2, 2, 3, 1) at f = 2, whose whole grad_mask (max|ref| 2e-7 ..
    2e-2) is the cancellation in d - sum wt d: 0.19, 1.5e-3, 2.8e-5 and 1.8e-4,
    the fp32 CPU closed form's own error on the same inputs;
  no defect found in the kernels; the file runs in 3.2 s (56 tests, the
  slowest 0.8 s).
Each parity test prints its band's largest error, the bound and the case.
"""
import numpy as np
import pytest

import upsample_sweep_util as usu
from golden_util import norm_err
from oracle import torch_ref
from upsample_bwd_ref import restated_backward

pytestmark = pytest.mark.gpu
DEV = "cuda"
REQUESTS = [(True, True), (True, False), (False, True)]      # (need_flow, need_mask)


def mismatches(got, want):
    bad = np.flatnonzero(np.asarray(got).reshape(-1) != np.asarray(want).reshape(-1))
    return f"{bad.size} of {np.asarray(want).size} elements differ, the first at flat index {int(bad[0])}" \
        if bad.size else ""


# ------------------------------------------------------------------ parity

@pytest.mark.parametrize("band", usu.BANDS, ids=usu.BAND_IDS)
def test_forward_elementwise(band):
    f, name = band
    worst = {s: (0.0, 0.0, None) for s in usu.SCALES}
    fails = []
    for n, case in enumerate(usu.bands(f)[name]):
        for scale in usu.SCALES:
            flow, mask, ref, S, fl, r_cpu = usu.fwd_case(case, scale)
            got = usu.guarded_upsample(DEV, flow, mask, f, phase=n % 2)
            r, bound = usu.elementwise_r(got, ref, S, fl), max(1e-5, 4 * r_cpu)
            if r >= worst[scale][0]:
                worst[scale] = (r, bound, case)
            if not r <= bound:
                fails.append((case, scale, r, bound))
    for s, (r, bound, case) in worst.items():
        print(f"f{f}-{name} scale {s:g}: worst r {r:.2e} (bound {bound:.2e}) at {case}")
    assert not fails, fails


@pytest.mark.parametrize("band", usu.BANDS, ids=usu.BAND_IDS)
def test_backward_parity(band):
    f, name = band
    worst = {(s, g): (0.0, 0.0, None) for s in usu.SCALES for g in ("grad_flow", "grad_mask")}
    fails = []
    for n, case in enumerate(usu.bands(f)[name]):
        for scale in usu.SCALES:
            flow, mask, gout, ref_flow, ref_mask = usu.bwd_case(case, scale)
            b_flow = b_mask = 1e-5
            if scale > 10:
                cpu_flow, cpu_mask = restated_backward(flow, mask, gout, f)          # fp32
                b_flow = max(1e-5, 4 * norm_err(cpu_flow.numpy(), ref_flow))
                b_mask = max(1e-5, 4 * norm_err(cpu_mask.numpy(), ref_mask))
            got = {rq: usu.guarded_upsample_backward(DEV, flow, mask, gout, f, *rq, phase=(n + k) % 2)
                   for k, rq in enumerate(REQUESTS)}
            g_flow, g_mask = got[REQUESTS[0]]
            e_flow, e_mask = norm_err(g_flow, ref_flow), norm_err(g_mask, ref_mask)
            for g, e, b in (("grad_flow", e_flow, b_flow), ("grad_mask", e_mask, b_mask)):
                if e >= worst[scale, g][0]:
                    worst[scale, g] = (e, b, case)
            if not (e_flow <= b_flow and e_mask <= b_mask):
                fails.append((case, scale, e_flow, b_flow, e_mask, b_mask))
            only_flow, none_mask = got[REQUESTS[1]]
            none_flow, only_mask = got[REQUESTS[2]]
            assert none_mask is None and none_flow is None
            assert np.array_equal(only_flow, g_flow), (case, scale, mismatches(only_flow, g_flow))
            assert np.array_equal(only_mask, g_mask), (case, scale, mismatches(only_mask, g_mask))
    for (s, g), (e, b, case) in worst.items():
        print(f"f{f}-{name} scale {s:g}: worst {g} {e:.2e} (bound {b:.2e}) at {case}")
    assert not fails, fails


# ----------------------------------------------------------------- routing

@pytest.mark.parametrize("f", usu.FACTORS)
def test_forward_routing_bit_exact(f):
    for n, shape in enumerate(usu.ROUTING_SHAPES):
        rc = usu.routing_case(shape + (f,), 100 * f + n)
        got = usu.guarded_upsample(DEV, rc["flow"], rc["mask"], f, phase=n % 2)
        assert np.array_equal(got, rc["out"]), (shape, f, mismatches(got, rc["out"]))


@pytest.mark.parametrize("f", usu.FACTORS)
def test_backward_routing_bit_exact(f):
    for n, shape in enumerate(usu.ROUTING_SHAPES):
        rc = usu.routing_case(shape + (f,), 100 * f + n)
        gflow, gmask = usu.guarded_upsample_backward(DEV, rc["flow_int"], rc["mask"], rc["gout_int"], f,
                                                     phase=n % 2)
        want = rc["gflow_int"].astype(np.float32)
        assert np.array_equal(want.astype(np.int64), rc["gflow_int"])
        assert np.array_equal(gflow, want), (shape, f, "grad_flow", mismatches(gflow, want))
        assert not gmask.any(), (shape, f, "grad_mask", mismatches(gmask, np.zeros_like(gmask)))
        # the forward on the integer flow, and grad_flow alone
        out = usu.guarded_upsample(DEV, rc["flow_int"], rc["mask"], f, phase=1 - n % 2)
        assert np.array_equal(out, rc["out_int"]), (shape, f, "out", mismatches(out, rc["out_int"]))
        only, _ = usu.guarded_upsample_backward(DEV, rc["flow_int"], rc["mask"], rc["gout_int"], f,
                                                need_mask=False, phase=1 - n % 2)
        assert np.array_equal(only, want), (shape, f, "grad_flow alone", mismatches(only, want))


# ------------------------------------------------------------------- phase

@pytest.mark.parametrize("case", usu.PHASE_CASES, ids=str)
def test_phase_independence(case):
    flow, mask, gout = usu.inputs(case, 2.0)
    f = case[4]
    a = (usu.guarded_upsample(DEV, flow, mask, f, phase=0),) + \
        usu.guarded_upsample_backward(DEV, flow, mask, gout, f, phase=0)
    b = (usu.guarded_upsample(DEV, flow, mask, f, phase=1),) + \
        usu.guarded_upsample_backward(DEV, flow, mask, gout, f, phase=1)
    for name, x, y in zip(("out", "grad_flow", "grad_mask"), a, b):
        assert np.array_equal(x, y), (name, mismatches(x, y))


# -------------------------------------------------------------- non-finite

@pytest.mark.parametrize("case", usu.NONFINITE_CASES, ids=str)
def test_nonfinite_masks(case):
    """-inf taps beside a finite one: weight 0, finite output inside the
    forward bound.  All nine taps -inf, or a +inf or a NaN among them: NaN in
    that sub-pixel's output elements (every channel), as the fp64 reference
    gives, and nowhere else."""
    N, C, H, W, f = case
    flow, mask, kind = usu.nonfinite_mask(case)
    ref, S, fl = usu.ref_forward(flow, mask, f), usu.ref_scale(flow, mask, f), usu.floor(flow, f)
    # what the reference does is what the generator meant
    nan_sub = np.broadcast_to((kind >= 4) & (kind <= 6), (C,) + kind.shape)          # c n i j h w
    nan_out = nan_sub.transpose(1, 0, 4, 2, 5, 3).reshape(N, C, f * H, f * W)
    assert np.array_equal(np.isnan(ref), nan_out) and np.isfinite(ref[~nan_out]).all()
    assert nan_out.any() and (~nan_out).any() and (kind < 4).any()
    for k in (4, 5, 6):
        assert (kind == k).any(), k
    cpu = torch_ref.convex_upsample(flow, mask, f).numpy()
    assert np.array_equal(np.isnan(cpu), nan_out)
    bound = max(1e-5, 4 * usu.elementwise_r(cpu, ref, S, fl, ~nan_out))
    got = usu.guarded_upsample(DEV, flow, mask, f, finite=False)
    assert np.array_equal(np.isnan(got), nan_out), mismatches(np.isnan(got), nan_out)
    assert np.isfinite(got[~nan_out]).all()
    r = usu.elementwise_r(got, ref, S, fl, ~nan_out)
    print(f"{case}: r {r:.2e} (bound {bound:.2e}), {int(nan_out.sum())} of {nan_out.size} NaN")
    assert r <= bound
