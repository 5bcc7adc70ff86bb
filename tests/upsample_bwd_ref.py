"""Shared by tests/test_upsample_backward_{cpu,gpu}.py: seeded inputs, the
fp64 autograd oracle (oracle/torch_ref.convex_upsample) and the closed-form
gradients of the convex upsampler written with plain torch ops.

With k = 3(dy+1)+(dx+1), wt = softmax_k(mask), nb = f * flow around the pixel
(zeros outside the image) and g = grad_out:
    d[n,k,i,j,h,w]  = sum_c g[n,c,i,j,h,w] * nb[n,c,k,h,w]
    grad_mask       = wt_k * (d_k - sum_k' wt_k' d_k')
    P[n,c,k,h,w]    = f * sum_{i,j} wt[n,k,i,j,h,w] * g[n,c,i,j,h,w]
    grad_flow[y,x]  = sum_k P[k][y - dy_k, x - dx_k]   (sources outside dropped)
"""
import functools

import torch
import torch.nn.functional as F

from oracle import torch_ref


def inputs(shape, mask_scale=2.0):
    """flow = randn*5, mask = randn*mask_scale, grad_out = randn (fp32, CPU)."""
    N, C, H, W, f = shape
    g = torch.Generator().manual_seed(11 + sum(shape))
    flow = torch.randn(N, C, H, W, generator=g) * 5
    mask = torch.randn(N, 9 * f * f, H, W, generator=g) * mask_scale
    gout = torch.randn(N, C, f * H, f * W, generator=g)
    return flow, mask, gout


def autograd_fp64(flow, mask, gout, f):
    """(grad_flow, grad_mask) of <torch_ref.convex_upsample, gout> in fp64."""
    fl = flow.double().requires_grad_(True)
    mk = mask.double().requires_grad_(True)
    torch_ref.convex_upsample(fl, mk, f).backward(gout.double())
    return fl.grad, mk.grad


@functools.lru_cache(maxsize=None)
def case(shape, mask_scale=2.0):
    """Inputs and their fp64 gradients, computed once per (shape, scale)."""
    flow, mask, gout = inputs(shape, mask_scale)
    return (flow, mask, gout) + autograd_fp64(flow, mask, gout, shape[4])


def restated_backward(flow, mask, gout, f):
    """The formulas above in the dtype of the arguments."""
    N, C, H, W = flow.shape
    wt = torch.softmax(mask.view(N, 9, f, f, H, W), dim=1)               # n k i j h w
    nb = F.unfold(f * flow, [3, 3], padding=1).view(N, C, 9, H, W)       # n c k h w
    g = gout.view(N, C, H, f, W, f).permute(0, 1, 3, 5, 2, 4)            # n c i j h w
    d = torch.einsum("ncijhw,nckhw->nkijhw", g, nb)
    grad_mask = (wt * (d - (wt * d).sum(1, keepdim=True))).reshape(N, 9 * f * f, H, W)
    P = F.pad(f * torch.einsum("nkijhw,ncijhw->nckhw", wt, g), (1, 1, 1, 1))
    grad_flow = torch.zeros_like(flow)
    for k in range(9):
        dy, dx = k // 3 - 1, k % 3 - 1
        grad_flow += P[:, :, k, 1 - dy:1 - dy + H, 1 - dx:1 - dx + W]
    return grad_flow, grad_mask
