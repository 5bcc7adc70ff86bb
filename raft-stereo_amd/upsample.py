"""Convex upsampler on the gfx950 kernel.

The reference's update block produces the mask (model.py:238-241, 0.25-scaled
at :264; f = 2**n_downsample at :236) but its truncated forward never uses it
(SURVEY Appendix A D8).  ``convex_upsample`` applies it the way RAFT-Stereo
does: softmax over the 9 neighbours for every sub-pixel, weighted sum of
f * flow over the low-resolution 3x3 neighbourhood (rc_convex_upsample,
include/raftcorr.h).  With ``differentiable=True`` it is an autograd function
whose backward is rc_convex_upsample_backward, for a training
loss on the full-resolution prediction.  No CPU fallback: HIP tensors only.
"""
import torch
from torch.autograd.function import once_differentiable

from . import _lib
from .corr import _require_hip, _stream


def _forward(f, m, factor):
    """The kernel on validated fp32 contiguous flow / mask."""
    N, C, H, W = f.shape
    out = torch.empty((N, C, factor * H, factor * W), dtype=torch.float32, device=f.device)
    if N * H * W == 0:
        return out
    with torch.cuda.device(f.device):
        rc = _lib.lib().rc_convex_upsample(f.data_ptr(), m.data_ptr(), N, C, H, W, factor,
                                           out.data_ptr(), _stream(f.device))
    _lib.check(rc, "rc_convex_upsample")
    return out


class _ConvexUpsample(torch.autograd.Function):
    """Saves the fp32 inputs only; the backward recomputes the softmax."""

    @staticmethod
    def forward(ctx, flow, mask, factor):
        f = flow.detach().float().contiguous()
        m = mask.detach().float().contiguous()
        ctx.save_for_backward(f, m)
        ctx.factor = factor
        ctx.dtypes = (flow.dtype, mask.dtype)
        return _forward(f, m, factor)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        f, m = ctx.saved_tensors
        need_flow, need_mask = ctx.needs_input_grad[:2]
        N, C, H, W = f.shape
        g = grad_out.float().contiguous()
        if g.data_ptr() % 16:               # a contiguous view at an odd storage offset
            g = g.clone()
        # the workspace holds the 9 C tap sums of every pixel between the two launches
        gf = torch.empty_like(f) if need_flow else None
        ws = torch.empty((N, C, 9, H, W), dtype=torch.float32, device=f.device) if need_flow else None
        gm = torch.empty_like(m) if need_mask else None
        if N * H * W:
            with torch.cuda.device(f.device):
                rc = _lib.lib().rc_convex_upsample_backward(
                    f.data_ptr(), m.data_ptr(), g.data_ptr(), N, C, H, W, ctx.factor,
                    gf.data_ptr() if need_flow else None, gm.data_ptr() if need_mask else None,
                    ws.data_ptr() if need_flow else None, _stream(f.device))
            _lib.check(rc, "rc_convex_upsample_backward")
        fdt, mdt = ctx.dtypes
        return (gf.to(fdt) if need_flow else None, gm.to(mdt) if need_mask else None, None)


def convex_upsample(flow, mask, factor, *, differentiable=False):
    """flow (N, C, H, W), mask (N, 9*factor**2, H, W) -> (N, C, factor*H, factor*W)
    fp32.  Inputs of other float dtypes are computed in fp32.

    ``differentiable=False`` is inference-only and raises when an input
    requires grad.  ``differentiable=True`` records an autograd node (first
    order only) that returns the gradients in the inputs' dtypes."""
    _require_hip(flow, "flow")
    _require_hip(mask, "mask")
    if not differentiable and torch.is_grad_enabled() and (flow.requires_grad or mask.requires_grad):
        raise RuntimeError("convex_upsample is inference-only unless differentiable=True; "
                           "pass it, or call under torch.no_grad()")
    if flow.device != mask.device:
        raise RuntimeError("convex_upsample: flow and mask on different devices")
    if flow.dim() != 4 or mask.dim() != 4:
        raise RuntimeError("convex_upsample: flow and mask must be 4-D")
    N, C, H, W = flow.shape
    if tuple(mask.shape) != (N, 9 * factor * factor, H, W):
        raise RuntimeError(f"convex_upsample: mask {tuple(mask.shape)} != "
                           f"{(N, 9 * factor * factor, H, W)}")
    if differentiable:
        return _ConvexUpsample.apply(flow, mask, factor)
    return _forward(flow.detach().float().contiguous(), mask.detach().float().contiguous(), factor)
