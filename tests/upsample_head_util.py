"""The case list, the guarded raw C-ABI caller and the references of the
upsampling head's tests (test_upsample_head_gpu.py, test_upsample_head_host.py),
on top of sweep_util.py's arena and upsample_sweep_util.py's references.

A case is (N, C, H, W, f): flow (N, C, H, W), mask (N, 9 f^2, H, W).  The
kernel (csrc/upsample_head.hip) runs one workgroup of f waves per 64 lane
groups; a lane group is one pixel, or in the planar class with 8-byte loads the
V = 4 (fp16 / bf16) or 2 (fp32) consecutive pixels of the flattened (h, w).
"""
import functools

import numpy as np
import torch

import sweep_util as su
import upsample_sweep_util as uu
from raft_stereo_amd import _lib

FACTORS = (1, 2, 4, 8)
DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
CODES = {"f32": _lib.RC_F32, "f16": _lib.RC_F16, "bf16": _lib.RC_BF16}
CLASSES = ("planar", "interleaved")
SCALES = (0.25, 1.0)                    # the kernel's `scale` argument
MASK_SCALES = uu.SCALES                 # mask = randn * 2 and randn * 40
WIDTHS = (1, 2, 3, 21, 22, 63, 64, 65, 70)
ODD = (1, 1, 2, 5)                      # run with the mask's base one element off its region's start


def shapes(f):
    """(N, C, H, W) of factor f, with the reason each is there."""
    out = [((2, 2, 3, W), "rows wrap inside a wave; taps in the neighbouring 64-pixel group") for W in WIDTHS]
    out += [((1, 1, 1, 1), "every neighbour outside the image"),
            ((3, 1, 1, 13), "several images in one group"),
            ((1, 1, 1, 256 // f + 1), "one lane past a 256-lane block")]
    return out


def cases(f):
    return [s + (f,) for s, _ in shapes(f)]


def es(dt):
    return 4 if dt == "f32" else 2


def vec(dt):
    """Pixels per lane of the planar class's 8-byte loads."""
    return 8 // es(dt)


def wide(case, dt, cls, base_off=0):
    """The launcher's choice (head_wide) for an arena mask of one image batch
    stride 9 f^2 H W: the arena's regions are 16-byte aligned."""
    N, C, H, W, f = case
    if cls == "interleaved":
        b = min(16, f * es(dt))
        return base_off % b == 0 and (9 * f * f * H * W * es(dt)) % b == 0
    return base_off % 8 == 0 and (H * W) % vec(dt) == 0 and (9 * f * f * H * W) % vec(dt) == 0


def groups(case, dt, cls, base_off=0):
    N, C, H, W, f = case
    return N * H * W // (vec(dt) if cls == "planar" and wide(case, dt, cls, base_off) else 1)


# ---------------------------------------------------------------- inputs

def rounded(mask, dt):
    """fp32 mask values rounded to the case's dtype (kept in fp32)."""
    return mask.to(DTYPES[dt]).float()


@functools.lru_cache(maxsize=None)
def case_inputs(case, mscale, dt):
    """(flow, mask in the case's dtype) -- upsample_sweep_util.inputs, the
    mask rounded once to dt."""
    flow, mask, _ = uu.inputs(case, mscale)
    return flow, mask.to(DTYPES[dt])


@functools.lru_cache(maxsize=None)
def reference(case, mscale, dt, scale):
    """(ref fp64, S, floor, r_cpu) on the widened, scaled mask."""
    flow, m = case_inputs(case, mscale, dt)
    m32 = scale * m.float()
    f = case[4]
    ref, S, fl = uu.ref_forward(flow, m32, f), uu.ref_scale(flow, m32, f), uu.floor(flow, f)
    r_cpu = uu.elementwise_r(uu.torch_ref.convex_upsample(flow, m32, f).numpy(), ref, S, fl)
    return ref, S, fl, r_cpu


def laid_out(mask, cls):
    """The mask's elements in memory order of its class, and its stride triple."""
    N, MC, H, W = mask.shape
    if cls == "planar":
        return mask.contiguous(), (MC * H * W, H * W, 1)
    return mask.permute(0, 2, 3, 1).contiguous(), (MC * H * W, 1, MC)


# ---------------------------------------------------------------- caller

def guarded_head(dev, flow, mask, f, dt, cls, scale, phase=0, base_off=0, flow_slice=False, finite=True):
    """rc_upsample_head on arena memory.  flow: fp32 CPU (N, C, H, W); mask:
    CPU tensor of the case's dtype, laid out here for ``cls``.  base_off: bytes
    between the mask region's start and the mask's first element (the region is
    that much larger, the slack holding zeros that must not be read into the
    result).  flow_slice: flow is passed as channels [0, C) of an (N, C + 1,
    H, W) tensor whose last channel is the arena's pattern-free NaN.  Returns
    out as numpy."""
    N, C, H, W = flow.shape
    assert tuple(mask.shape) == (N, 9 * f * f, H, W) and mask.dtype == DTYPES[dt]
    mem, ms = laid_out(mask, cls)
    raw = mem.reshape(-1).view(torch.uint8)
    if base_off:
        raw = torch.cat([torch.zeros(base_off, dtype=torch.uint8), raw])
    if flow_slice:
        fl = torch.cat([flow, torch.full((N, 1, H, W), float("nan"))], dim=1).contiguous()
        fs = ((C + 1) * H * W, H * W)
    else:
        fl, fs = flow.contiguous(), (C * H * W, H * W)
    oshape = (N, C, f * H, f * W)
    ar = su.arena(dev, [("flow", fl.numel() * 4, fl), ("mask", raw.numel(), raw),
                        ("out", int(np.prod(oshape)) * 4, None)], phase, bf16=False)
    rc = _lib.lib().rc_upsample_head(ar.ptr("flow"), _lib.long_array(fs), ar.ptr("mask") + base_off,
                                     _lib.long_array(ms), CODES[dt], scale, N, C, H, W, f, ar.ptr("out"), None)
    _lib.check(rc, "rc_upsample_head")
    ar.assert_guards_intact()
    ar.assert_outputs_written(["out"])
    out = ar.region("out", np.float32).reshape(oshape).copy()
    if finite:
        assert np.isfinite(out).all(), "non-finite output"
    return out


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)
