"""rc_convex_upsample_backward through ``convex_upsample(differentiable=True)``
(DESIGN.md §3.6): both gradients against fp64 CPU autograd of
oracle/torch_ref.convex_upsample (pinned to the closed form by
tests/test_upsample_backward_cpu.py).

Bound: golden_util.norm_err <= 1e-5 per gradient, the forward's bound in
tests/test_upsample.py (fp32 CPU evaluation of the closed form reaches
<= 4.3e-7 on these inputs, so a wrong tap cannot hide).  With a saturated
softmax (mask = randn * 40) the closed form's own fp32 error grows through
the cancellation in d - sum wt d, so there the bound is max(1e-5, 4 x that
error on the same inputs)."""
import ctypes

import pytest
import torch

from golden_util import norm_err
from upsample_bwd_ref import case, inputs, restated_backward

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1, 1, 4),      # every neighbour outside the image
          (1, 2, 1, 5, 2),      # H = 1
          (2, 1, 5, 1, 8),      # W = 1
          (2, 2, 7, 9, 4),      # odd H and W
          (1, 1, 16, 20, 2),    # f = 2
          (1, 2, 5, 5, 8),      # f = 8, C = 2
          (3, 1, 10, 13, 1),    # f = 1
          (1, 1, 19, 70, 4),    # taps from another workgroup's 64 pixels
          (1, 3, 33, 17, 4)]    # C = 3, rows wrap inside a wave
IDS = ["x".join(map(str, s)) for s in SHAPES]


def hip_grads(flow, mask, gout, f, need_flow=True, need_mask=True):
    """Gradients of <convex_upsample(flow, mask), gout> on the GPU; ``gout``
    None means out.sum().backward()."""
    from raft_stereo_amd.upsample import convex_upsample
    fl = flow.cuda().requires_grad_(need_flow)
    mk = mask.cuda().requires_grad_(need_mask)
    out = convex_upsample(fl, mk, f, differentiable=True)
    if gout is None:
        out.sum().backward()
    else:
        out.backward(gout.cuda())
    return fl.grad, mk.grad


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_parity_vs_fp64_autograd(shape):
    flow, mask, gout, ref_flow, ref_mask = case(shape)
    got_flow, got_mask = hip_grads(flow, mask, gout, shape[4])
    e_flow = norm_err(got_flow.cpu().numpy(), ref_flow.numpy())
    e_mask = norm_err(got_mask.cpu().numpy(), ref_mask.numpy())
    print(f"{shape}: grad_flow {e_flow:.2e} grad_mask {e_mask:.2e}")
    assert got_flow.shape == flow.shape and got_flow.dtype == torch.float32
    assert got_mask.shape == mask.shape and got_mask.dtype == torch.float32
    assert e_flow <= 1e-5 and e_mask <= 1e-5


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_saturated_softmax(shape):
    flow, mask, gout, ref_flow, ref_mask = case(shape, 40.0)
    cpu_flow, cpu_mask = restated_backward(flow, mask, gout, shape[4])      # fp32
    b_flow = max(1e-5, 4 * norm_err(cpu_flow.numpy(), ref_flow.numpy()))
    b_mask = max(1e-5, 4 * norm_err(cpu_mask.numpy(), ref_mask.numpy()))
    got_flow, got_mask = hip_grads(flow, mask, gout, shape[4])
    assert torch.isfinite(got_flow).all() and torch.isfinite(got_mask).all()
    e_flow = norm_err(got_flow.cpu().numpy(), ref_flow.numpy())
    e_mask = norm_err(got_mask.cpu().numpy(), ref_mask.numpy())
    print(f"{shape}: grad_flow {e_flow:.2e} (bound {b_flow:.2e}) "
          f"grad_mask {e_mask:.2e} (bound {b_mask:.2e})")
    assert e_flow <= b_flow and e_mask <= b_mask


@pytest.mark.parametrize("shape", [(2, 2, 7, 9, 4), (1, 1, 19, 70, 4)], ids=str)
def test_needs_input_grad(shape):
    flow, mask, gout = inputs(shape)
    both_flow, both_mask = hip_grads(flow, mask, gout, shape[4])
    only_flow, none_mask = hip_grads(flow, mask, gout, shape[4], need_mask=False)
    none_flow, only_mask = hip_grads(flow, mask, gout, shape[4], need_flow=False)
    assert none_mask is None and none_flow is None
    assert torch.equal(only_flow, both_flow)
    assert torch.equal(only_mask, both_mask)


def test_repeated_runs_are_bit_equal():
    shape = (1, 1, 19, 70, 4)
    flow, mask, gout = inputs(shape)
    a_flow, a_mask = hip_grads(flow, mask, gout, 4)
    b_flow, b_mask = hip_grads(flow, mask, gout, 4)
    assert torch.equal(a_flow, b_flow) and torch.equal(a_mask, b_mask)


def test_expanded_grad_out():
    """out.sum().backward() hands the node a stride-0 gradient."""
    shape = (2, 2, 7, 9, 4)
    flow, mask, gout = inputs(shape)
    s_flow, s_mask = hip_grads(flow, mask, None, 4)
    o_flow, o_mask = hip_grads(flow, mask, torch.ones_like(gout), 4)
    assert torch.equal(s_flow, o_flow) and torch.equal(s_mask, o_mask)


@pytest.mark.parametrize("f", [2, 4])
def test_unaligned_grad_out(f):
    """A contiguous grad_out one float into its storage: 4 mod 16 bytes, which
    rc_convex_upsample_backward refuses at f >= 2 (its vector load); the
    wrapper hands the kernel an aligned copy."""
    shape = (2, 2, 7, 9, f)
    flow, mask, gout = inputs(shape)
    store = torch.empty(gout.numel() + 5, device="cuda")
    lead = (4 - store.data_ptr() % 16) % 16 // 4                   # floats to an address 4 mod 16
    g = store[lead:lead + gout.numel()].view(gout.shape)
    g.copy_(gout)
    assert g.is_contiguous() and g.data_ptr() % 16 == 4
    from raft_stereo_amd.upsample import convex_upsample
    fl = flow.cuda().requires_grad_(True)
    mk = mask.cuda().requires_grad_(True)
    convex_upsample(fl, mk, f, differentiable=True).backward(g)
    a_flow, a_mask = hip_grads(flow, mask, gout, f)
    assert torch.equal(fl.grad, a_flow) and torch.equal(mk.grad, a_mask)


def test_empty_batch():
    from raft_stereo_amd.upsample import convex_upsample
    fl = torch.empty(0, 2, 7, 9, device="cuda").requires_grad_(True)
    mk = torch.empty(0, 9 * 16, 7, 9, device="cuda").requires_grad_(True)
    out = convex_upsample(fl, mk, 4, differentiable=True)
    assert out.shape == (0, 2, 28, 36) and out.grad_fn is not None
    out.sum().backward()
    assert fl.grad.shape == fl.shape and mk.grad.shape == mk.shape


def test_bf16_mask_gets_bf16_gradient():
    shape = (2, 2, 7, 9, 4)
    flow, mask, gout = inputs(shape)
    mask16 = mask.bfloat16()
    flow_g, mask_g = hip_grads(flow, mask16, gout, 4)
    ref_flow, ref_mask = hip_grads(flow, mask16.float(), gout, 4)
    assert mask_g.dtype == torch.bfloat16 and flow_g.dtype == torch.float32
    assert torch.equal(mask_g, ref_mask.bfloat16())
    assert torch.equal(flow_g, ref_flow)


def test_capi_validation():
    from raft_stereo_amd import _lib
    L = _lib.lib()
    p = lambda a: ctypes.c_void_p(a)  # noqa: E731
    call = lambda N, f, gf, gm, ws: L.rc_convex_upsample_backward(  # noqa: E731
        p(0x1000), p(0x2000), p(0x3000), N, 1, 4, 4, f, gf, gm, ws, None)
    assert call(1, 4, None, None, p(0x6000)) == _lib.RC_EINVAL       # nothing requested
    assert L.rc_last_error()
    assert call(1, 4, p(0x4000), p(0x5000), None) == _lib.RC_EINVAL  # grad_flow without workspace
    assert b"workspace" in L.rc_last_error()
    assert call(1, 3, p(0x4000), p(0x5000), p(0x6000)) == _lib.RC_EUNSUPPORTED
    assert b"factor" in L.rc_last_error()
    assert call(0, 4, p(0x4000), p(0x5000), p(0x6000)) == _lib.RC_OK  # empty: nothing launched


def test_network_trains_on_full_resolution_predictions():
    """With grad enabled ``upsample=True`` gives differentiable predictions;
    the loss reaches the mask head and, through the corr path, the feature
    encoder.  (No numeric comparison here: parity is pinned at function
    level, where the inputs are identical.)"""
    from raft_stereo_amd.network import RAFTStereo, StereoArgs
    torch.manual_seed(0)
    model = RAFTStereo(StereoArgs()).train().cuda()
    g = torch.Generator().manual_seed(8)
    img1 = (torch.rand(1, 3, 64, 96, generator=g) * 255).cuda()
    img2 = torch.roll(img1, -4, dims=-1)
    preds = model(img1, img2, iters=2, upsample=True)
    assert len(preds) == 2
    for pr in preds:
        assert pr.grad_fn is not None and pr.shape == (1, 1, 64, 96)
    sum(pr.abs().mean() for pr in preds).backward()
    for w in (model.update_block.mask[2].weight, model.conv2[1].weight):
        assert w.grad is not None and torch.isfinite(w.grad).all()
        assert w.grad.abs().max() > 0
