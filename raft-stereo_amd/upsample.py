"""Convex upsampler on the gfx950 kernel.

The reference's update block produces the mask (model.py:238-241, 0.25-scaled
at :264; f = 2**n_downsample at :236) but its truncated forward never uses it
(SURVEY Appendix A D8).  ``convex_upsample`` applies it the way RAFT-Stereo
does: softmax over the 9 neighbours for every sub-pixel, weighted sum of
f * flow over the low-resolution 3x3 neighbourhood (rc_convex_upsample,
include/raftcorr.h).  With ``differentiable=True`` it is an autograd function
whose backward is rc_convex_upsample_backward, for a training
loss on the full-resolution prediction.  No CPU fallback: HIP tensors only.

``upsample_head`` is the same upsampler for the last step of an inference
forward (rc_upsample_head): it reads the mask as the update
block's last convolution wrote it -- fp32, fp16 or bf16, NCHW or
channels-last, unscaled -- and applies the 0.25 inside the kernel, so the
scale, cast and layout passes in front of ``convex_upsample`` do not run.
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


_MASK_CODES = {torch.float32: _lib.RC_F32, torch.float16: _lib.RC_F16, torch.bfloat16: _lib.RC_BF16}


def upsample_head(flow, mask, factor, scale=0.25):
    """flow (N, C, H, W), mask (N, 9*factor**2, H, W) of unscaled logits ->
    (N, C, factor*H, factor*W) fp32: ``convex_upsample(flow, scale *
    mask.float(), factor)`` bit for bit, in one launch that reads the mask in
    its own dtype (float32, float16 or bfloat16) and layout (NCHW- or
    channels-last-dense; anything else is made contiguous first).  The flow is
    computed in fp32; a channel slice of a wider tensor is passed by its
    strides, not copied.

    Inference only: raises when grad is enabled and an input requires grad;
    use ``convex_upsample(..., differentiable=True)`` for a loss on the
    full-resolution prediction."""
    _require_hip(flow, "flow")
    _require_hip(mask, "mask")
    if torch.is_grad_enabled() and (flow.requires_grad or mask.requires_grad):
        raise RuntimeError("upsample_head is inference-only; call it under torch.no_grad(), or use "
                           "convex_upsample(..., differentiable=True)")
    if flow.device != mask.device:
        raise RuntimeError("upsample_head: flow and mask on different devices")
    if flow.dim() != 4 or mask.dim() != 4:
        raise RuntimeError("upsample_head: flow and mask must be 4-D")
    N, C, H, W = flow.shape
    if tuple(mask.shape) != (N, 9 * factor * factor, H, W):
        raise RuntimeError(f"upsample_head: mask {tuple(mask.shape)} != "
                           f"{(N, 9 * factor * factor, H, W)}")
    if mask.dtype not in _MASK_CODES:
        raise RuntimeError(f"upsample_head: mask dtype {mask.dtype}: float32, float16 or bfloat16")
    if not flow.is_floating_point() or flow.dtype == torch.float64:
        raise RuntimeError(f"upsample_head: flow dtype {flow.dtype}: float32, float16 or bfloat16")
    f = flow.detach().float()
    if N * H * W and (f.stride(3) != 1 or f.stride(2) != W):     # rows of W unit-stride elements, H of them dense
        f = f.contiguous()
    m = mask.detach()
    MC = 9 * factor * factor
    planar = m.stride()[1:] == (H * W, W, 1)
    inter = m.stride()[1:] == (1, W * MC, MC)
    if N * H * W and not (planar or inter):
        m = m.contiguous()
        inter = False
    out = torch.empty((N, C, factor * H, factor * W), dtype=torch.float32, device=f.device)
    if N * H * W == 0:
        return out
    ms = (m.stride(0), 1, MC) if inter and not m.is_contiguous() else (m.stride(0), H * W, 1)
    with torch.cuda.device(f.device):
        rc = _lib.lib().rc_upsample_head(f.data_ptr(), _lib.long_array([f.stride(0), f.stride(1)]), m.data_ptr(),
                                         _lib.long_array(ms), _MASK_CODES[m.dtype], float(scale), N, C, H, W,
                                         factor, out.data_ptr(), _stream(f.device))
    _lib.check(rc, "rc_upsample_head")
    return out
