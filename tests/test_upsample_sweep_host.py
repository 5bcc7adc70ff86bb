"""Host-side companion of test_upsample_sweep_gpu.py (no GPU): the one-hot
routing expectations are the formula's, the sweep lists reach the block edges
the GPU file's docstring claims, and the elementwise forward bound cannot grow
past its analytic cap on any sweep input."""
import numpy as np
import pytest
import torch

import upsample_sweep_util as usu
from oracle import torch_ref
from test_upsample import loop_upsample
from upsample_bwd_ref import autograd_fp64

SMALL = (2, 2, 3, 4)


# ---------------------------------------------------------------- routing

def test_one_hot_softmax_is_exact_in_fp32():
    """expf(-200) is 0 in fp32, so the routing mask's weights are exactly
    one-hot and the fp32 restatement reproduces the gather bit for bit."""
    assert float(torch.exp(torch.tensor(usu.OFF, dtype=torch.float32))) == 0.0
    for f in usu.FACTORS:
        rc = usu.routing_case(SMALL + (f,), f)
        wt = torch.softmax(rc["mask"].view(2, 9, f, f, 3, 4), dim=1).numpy()
        assert set(np.unique(wt)) == {0.0, 1.0}
        assert np.array_equal(wt.argmax(1), rc["sel"])
        assert np.array_equal(torch_ref.convex_upsample(rc["flow"], rc["mask"], f).numpy(), rc["out"])


@pytest.mark.parametrize("f", usu.FACTORS)
def test_routing_expectation_is_the_formula(f):
    """The numpy gather / scatter against the fp64 loop of the formula and
    fp64 autograd, exactly: both sides are integers.  e^-200 is 0 in fp32 but
    1.4e-87 in fp64, so the fp64 sides get the mask x 4 (0 and -800: e^-800 is
    0 in fp64 too), which selects the same taps."""
    rc = usu.routing_case(SMALL + (f,), 10 + f)
    assert rc["sel"].min() == 0 and rc["sel"].max() == 8
    mask4 = rc["mask"] * 4
    want = loop_upsample(rc["flow_int"].numpy(), mask4.numpy(), f)
    assert np.array_equal(rc["out_int"], want) and 0 < np.abs(want).max() <= 8 * f
    gflow, gmask = autograd_fp64(rc["flow_int"], mask4, rc["gout_int"], f)
    assert np.array_equal(rc["gflow_int"], gflow.numpy()) and np.abs(gflow.numpy()).max() > 0
    assert not gmask.numpy().any()
    # taps outside the image are selected too, and give 0
    N, C, H, W = SMALL
    h, w = np.arange(H).reshape(1, 1, 1, H, 1), np.arange(W)
    yy, xx = h + rc["sel"] // 3 - 1, w + rc["sel"] % 3 - 1
    assert ((yy < 0) | (yy >= H) | (xx < 0) | (xx >= W)).any()
    # the arbitrary-valued expectation holds nothing but f * flow and the zeros of the padding
    assert set(np.unique(rc["out"])) <= set(np.unique(f * rc["flow"].numpy())) | {0.0}


def test_routing_backward_sums_are_exact_in_fp32():
    """|P| <= 8 f^3 and nine of them stay under 2^24."""
    assert 9 * 8 * max(usu.FACTORS) ** 3 < 2 ** 24
    for shape in usu.ROUTING_SHAPES:
        rc = usu.routing_case(shape + (8,), 1)
        assert np.abs(rc["gflow_int"]).max() < 2 ** 24
        for k in ("flow_int", "gout_int"):
            v = rc[k].numpy()
            assert np.array_equal(v, np.round(v)) and np.abs(v).max() <= 8


# --------------------------------------------------------------- coverage

def test_every_factor_in_every_sweep():
    assert usu.FACTORS == (1, 2, 4, 8)
    assert {f for f, _ in usu.BANDS} == set(usu.FACTORS)
    for cs in (usu.PHASE_CASES, usu.NONFINITE_CASES):
        assert [c[4] for c in cs] == list(usu.FACTORS)
    for f in usu.FACTORS:
        cs = usu.cases(f)
        assert len(cs) == len(set(cs)) and all(c[4] == f for c in cs)
        assert sum(usu.bands(f).values(), []) == cs
        for W in range(1, 71):
            assert (2, 2, 3, W, f) in cs
        for H in range(1, 10):
            assert (2, 1, H, 5, f) in cs
        for N in range(1, 6):
            assert (N, 3, 1, 13, f) in cs
        for C in range(1, 5):
            assert (2, C, 3, 11, f) in cs


@pytest.mark.parametrize("f", usu.FACTORS)
def test_forward_block_edges(f):
    """N H f W lanes in blocks of 256.  The lane count is a multiple of f, so
    the tails nearest to a block edge are f lanes and 256 - f lanes (1 and
    255 at f = 1), besides the full block."""
    tot = [usu.totals(c)[0] for c in usu.cases(f)]
    assert all(t % f == 0 for t in tot)
    assert {0, f, 256 - f} <= {t % 256 for t in tot}
    if f == 1:
        assert {0, 1, 255} <= {t % 256 for t in tot}
    assert any(t > 256 for t in tot) and any(t > 256 and t % 256 for t in tot)
    assert [usu.totals(c + (f,))[0] for c in usu.fwd_edges(f)] == [256, 256 + f, 512 - f]


@pytest.mark.parametrize("f", usu.FACTORS)
def test_backward_block_edges(f):
    """N H W pixels in workgroups of 64."""
    cs = usu.cases(f)
    tot = [usu.totals(c)[1] for c in cs]
    assert {0, 1, 63} <= {t % 64 for t in tot}
    assert any((t + 63) // 64 >= 4 for t in tot)
    # one 64-pixel block with pixels of three or more images
    assert any(N >= 3 and H * W < 32 and 64 // (H * W) >= 2 for N, C, H, W, _ in cs)
    # the gather: N C H W lanes in blocks of 256, more than one block
    assert any(N * C * H * W > 256 for N, C, H, W, _ in cs)


@pytest.mark.parametrize("f", usu.FACTORS)
def test_degenerate_shapes_and_channels(f):
    cs = usu.cases(f)
    assert any(H == 1 and W > 1 for _, _, H, W, _ in cs)
    assert any(W == 1 and H > 1 for _, _, H, W, _ in cs)
    assert any(H == 1 and W == 1 for _, _, H, W, _ in cs)
    assert {C for _, C, _, _, _ in cs} == {1, 2, 3, 4}
    assert {N for N, _, _, _, _ in cs} == {1, 2, 3, 4, 5}
    # the largest mask is under 1 MB
    assert max(N * 9 * f * f * H * W * 4 for N, _, H, W, _ in cs) < 1_000_000


def test_routing_shapes():
    assert usu.ROUTING_SHAPES == [(2, 2, 3, 7), (1, 1, 1, 1), (3, 1, 1, 13), (1, 2, 5, 66)]


# ---------------------------------------------------------- tolerance cap

def test_cap_is_the_analytic_fp32_bound():
    assert usu.R_FP32_MAX == pytest.approx((87.34 + 23) * 2.0 ** -24, rel=1e-4)
    assert 2.6e-5 < usu.CAP < 2.7e-5
    # a weight survives in fp32 only for d < 126 ln 2
    assert float(torch.exp(torch.tensor(-87.3, dtype=torch.float32))) >= 2.0 ** -126
    assert float(torch.exp(torch.tensor(-87.4, dtype=torch.float32))) < 2.0 ** -126


@pytest.mark.parametrize("scale", usu.SCALES)
@pytest.mark.parametrize("f", usu.FACTORS)
def test_cpu_restatement_stays_under_the_cap(f, scale):
    """The GPU bound is max(1e-5, 4 r_cpu): on every sweep input 4 r_cpu stays
    under the cap, so no input can buy the kernel more than 2.63e-5."""
    worst = max(usu.fwd_case(c, scale)[5] for c in usu.cases(f))
    print(f"f = {f}, scale {scale}: worst r_cpu {worst:.2e} (R_FP32_MAX {usu.R_FP32_MAX:.2e})")
    assert 4 * worst <= usu.CAP
    for c in usu.NONFINITE_CASES + usu.PHASE_CASES:
        if c[4] == f:
            assert 4 * usu.fwd_case(c, scale)[5] <= usu.CAP
