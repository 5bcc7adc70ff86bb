"""Convex upsampler.

The reference builds the upsampling mask (model.py:238-241, :264) but its
truncated forward never applies it, so there is no reference output to pin:
the oracle is oracle/torch_ref.convex_upsample (RAFT-Stereo's F.unfold +
softmax formulation), itself checked here against an explicit per-pixel loop
of the formula ("parity unpinned" by the reference).
Tolerance for the HIP kernel: max|d|/max|ref| <= 1e-5 (expf and summation
order differ from torch's softmax)."""
import numpy as np
import pytest
import torch

from golden_util import norm_err
from oracle import torch_ref


def loop_upsample(flow, mask, f):
    N, C, H, W = flow.shape
    out = np.zeros((N, C, f * H, f * W), np.float64)
    fl = np.pad(flow.astype(np.float64), ((0, 0), (0, 0), (1, 1), (1, 1)))
    m = mask.astype(np.float64).reshape(N, 9, f, f, H, W)
    for n in range(N):
        for h in range(H):
            for w in range(W):
                for i in range(f):
                    for j in range(f):
                        e = np.exp(m[n, :, i, j, h, w] - m[n, :, i, j, h, w].max())
                        wgt = e / e.sum()
                        for c in range(C):
                            nb = fl[n, c, h:h + 3, w:w + 3].reshape(9)
                            out[n, c, f * h + i, f * w + j] = (wgt * f * nb).sum()
    return out


@pytest.mark.parametrize("shape", [(1, 2, 3, 4, 2), (2, 1, 4, 3, 4)], ids=str)
def test_restatement_matches_formula(shape):
    N, C, H, W, f = shape
    g = torch.Generator().manual_seed(sum(shape))
    flow = torch.randn(N, C, H, W, generator=g) * 3
    mask = torch.randn(N, 9 * f * f, H, W, generator=g) * 2
    got = torch_ref.convex_upsample(flow, mask, f).double().numpy()
    assert norm_err(got, loop_upsample(flow.numpy(), mask.numpy(), f)) <= 1e-6


SHAPES = [(2, 2, 7, 9, 4), (1, 1, 16, 20, 2), (1, 2, 5, 5, 8), (3, 1, 10, 13, 1),
          (8, 1, 135, 240, 4)]


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_hip_vs_restatement(shape):
    from raft_stereo_amd.upsample import convex_upsample
    N, C, H, W, f = shape
    g = torch.Generator().manual_seed(3 + sum(shape))
    flow = torch.randn(N, C, H, W, generator=g) * 5
    mask = torch.randn(N, 9 * f * f, H, W, generator=g) * 2
    got = convex_upsample(flow.cuda(), mask.cuda(), f).cpu()
    ref = torch_ref.convex_upsample(flow, mask, f)
    assert got.shape == ref.shape
    assert norm_err(got.numpy(), ref.numpy()) <= 1e-5


@pytest.mark.gpu
def test_network_full_resolution_output():
    """RAFTStereo(..., upsample=True): every prediction is the full-resolution
    x-flow, a convex combination of f x the low-resolution flow around it."""
    from raft_stereo_amd.network import RAFTStereo, StereoArgs
    torch.manual_seed(0)
    model = RAFTStereo(StereoArgs()).eval().cuda()
    g = torch.Generator().manual_seed(8)
    img1 = (torch.rand(1, 3, 64, 96, generator=g) * 255).cuda()
    img2 = torch.roll(img1, -4, dims=-1)
    with torch.no_grad():
        low = model(img1, img2, iters=3)
        up = model(img1, img2, iters=3, upsample=True)
    assert len(up) == 3 and up[-1].shape == (1, 1, 64, 96)
    assert torch.isfinite(up[-1]).all()
    f = 4
    lo = low[-1][:, :1]
    pad = torch.nn.functional.pad(lo, (1, 1, 1, 1))
    nb = torch.nn.functional.unfold(pad, 3).view(1, 9, 16, 24) * f
    hi_max = nb.max(1).values.repeat_interleave(f, 1).repeat_interleave(f, 2)
    hi_min = nb.min(1).values.repeat_interleave(f, 1).repeat_interleave(f, 2)
    # allow the MIOpen run-to-run spread between the two forward passes
    assert (up[-1][0, 0] <= hi_max[0] + 1e-3).all() and (up[-1][0, 0] >= hi_min[0] - 1e-3).all()


def test_capi_alignment_validation():
    """The forward stores, and the backward loads, the f values of a sub-row
    as one vector: out and grad_out must be aligned to 4 min(f, 4) bytes, and
    a pointer that is not gives RC_EINVAL before anything is launched (the
    fabricated addresses are never dereferenced).  No GPU needed."""
    import ctypes

    from raft_stereo_amd import _lib
    L = _lib.lib()
    p = lambda a: ctypes.c_void_p(a)  # noqa: E731
    fwd = lambda N, f, out: L.rc_convex_upsample(p(0x1000), p(0x2000), N, 1, 4, 4, f, p(out), None)  # noqa: E731
    bwd = lambda N, f, gout: L.rc_convex_upsample_backward(  # noqa: E731
        p(0x1000), p(0x2000), p(gout), N, 1, 4, 4, f, p(0x4000), p(0x5000), p(0x6000), None)
    for call, what in ((fwd, b"out"), (bwd, b"grad_out")):
        for f, offs in ((2, (4,)), (4, (4, 8, 12)), (8, (4, 8, 12))):
            for off in offs:
                assert call(1, f, 0x3000 + off) == _lib.RC_EINVAL, (what, f, off)
                err = L.rc_last_error()
                assert b"aligned" in err and what + b" must be %d-byte" % (4 * min(f, 4)) in err, err
        # factor 1: any 4-byte-aligned pointer passes validation (N = 0: nothing is launched)
        for off in (0, 4, 8, 12):
            assert call(0, 1, 0x3000 + off) == _lib.RC_OK, (what, off)
            assert not L.rc_last_error()


WRAP = (2, 1, 7, 9, 4)


def _wrap_inputs():
    N, C, H, W, f = WRAP
    g = torch.Generator().manual_seed(41)
    p = (torch.randn(N, 2, H, W, generator=g) * 5).cuda()
    mask = (torch.randn(N, 9 * f * f, H, W, generator=g) * 2).cuda()
    return p, mask, f


@pytest.mark.gpu
def test_wrapper_takes_the_network_slice():
    """RAFTStereo hands over flow = p[:, :1] of a two-channel tensor."""
    from raft_stereo_amd.upsample import convex_upsample
    p, mask, f = _wrap_inputs()
    flow = p[:, :1]
    assert not flow.is_contiguous()
    want = convex_upsample(flow.float().contiguous(), mask, f)
    assert torch.equal(convex_upsample(flow, mask, f), want)
    assert norm_err(want.cpu().numpy(), torch_ref.convex_upsample(flow.cpu(), mask.cpu(), f).numpy()) <= 1e-5


@pytest.mark.gpu
def test_wrapper_takes_channels_last():
    from raft_stereo_amd.upsample import convex_upsample
    p, mask, f = _wrap_inputs()
    want = convex_upsample(p.contiguous(), mask, f)
    p_cl, mask_cl = p.to(memory_format=torch.channels_last), mask.to(memory_format=torch.channels_last)
    assert not p_cl.is_contiguous() and not mask_cl.is_contiguous()
    assert torch.equal(convex_upsample(p_cl, mask_cl, f), want)
    assert torch.equal(convex_upsample(p_cl[:, :1], mask_cl, f), want[:, :1])


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=str)
def test_wrapper_takes_16_bit_inputs(dtype):
    from raft_stereo_amd.upsample import convex_upsample
    p, mask, f = _wrap_inputs()
    flow16, mask16 = p[:, :1].to(dtype), mask.to(dtype)
    want = convex_upsample(flow16.float().contiguous(), mask16.float().contiguous(), f)
    got = convex_upsample(flow16, mask16, f)
    assert got.dtype == torch.float32 and torch.equal(got, want)
    assert torch.equal(convex_upsample(flow16, mask16.float(), f), want)
    assert torch.equal(convex_upsample(flow16.float(), mask16, f), want)


@pytest.mark.gpu
@pytest.mark.parametrize("differentiable", [False, True])
def test_wrapper_empty_batch(differentiable):
    from raft_stereo_amd.upsample import convex_upsample
    flow = torch.empty(0, 2, 7, 9).cuda()
    mask = torch.empty(0, 9 * 16, 7, 9).cuda()
    out = convex_upsample(flow, mask, 4, differentiable=differentiable)
    assert out.shape == (0, 2, 28, 36) and out.dtype == torch.float32 and out.is_cuda
