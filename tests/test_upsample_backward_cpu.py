"""The closed-form gradients of the convex upsampler (DESIGN.md §3.6,
tests/upsample_bwd_ref.py) equal fp64 autograd of
oracle/torch_ref.convex_upsample.  This pins the oracle the GPU tests of
rc_convex_upsample_backward use; no GPU needed.

Bound: 1e-12 normalised (max|d| / max|ref|) in fp64 -- both sides are a few
dozen fp64 operations per element, four orders above their rounding."""
import pytest

from golden_util import norm_err
from upsample_bwd_ref import case, restated_backward

SHAPES = [(1, 1, 1, 1, 4), (1, 2, 1, 5, 2), (2, 1, 5, 1, 8), (2, 2, 7, 9, 4), (3, 1, 10, 13, 1)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_formulas_match_fp64_autograd(shape):
    flow, mask, gout, ref_flow, ref_mask = case(shape)
    got_flow, got_mask = restated_backward(flow.double(), mask.double(), gout.double(), shape[4])
    e_flow = norm_err(got_flow.numpy(), ref_flow.numpy())
    e_mask = norm_err(got_mask.numpy(), ref_mask.numpy())
    print(f"{shape}: grad_flow {e_flow:.2e} grad_mask {e_mask:.2e}")
    assert got_flow.shape == flow.shape and got_mask.shape == mask.shape
    assert e_flow <= 1e-12 and e_mask <= 1e-12
