"""float64 numpy evaluation of the three modes of rc_gru_assemble (copy,
pool2x, bilinear): the reference of tests/test_gru_inputs_gpu.py.  Inputs
(N, C, H, W) are widened to float64.

The bilinear source coordinates are fp32 by definition (ATen's formula: the
scale, the coordinate, its integer part and the two weights are fp32 values),
so they are computed in fp32 and then widened; the interpolation itself and
the pooling sum are float64.  A reference with exact rational coordinates
differs from ATen by 8.7e-6 at 135x240 -- the coordinates' rounding, not the
kernel's -- and is not used."""
import numpy as np


def copy(src):
    return np.asarray(src, np.float64)


def pool2x(src):
    """3x3 average, stride 2, zero padding 1, the padding counted: sum / 9."""
    x = np.asarray(src, np.float64)
    N, C, H, W = x.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    pad = np.zeros((N, C, 2 * Ho + 1, 2 * Wo + 1))
    pad[:, :, 1:H + 1, 1:W + 1] = x
    acc = np.zeros((N, C, Ho, Wo))
    for kh in range(3):
        for kw in range(3):
            acc += pad[:, :, kh:kh + 2 * Ho:2, kw:kw + 2 * Wo:2]
    return acc / 9.0


def axis(S, D):
    """(i0, i1, l0, l1) of the D destination indices over a source of size S:
    fp32 arithmetic, the weights widened to float64."""
    f = np.float32
    scale = f(S - 1) / f(D - 1) if D > 1 else f(0.0)
    s = (scale * np.arange(D, dtype=np.float32)).astype(np.float32)
    i0 = s.astype(np.int64)
    i1 = i0 + (i0 < S - 1)
    l1 = (s - i0.astype(np.float32)).astype(np.float32)
    l0 = (f(1.0) - l1).astype(np.float32)
    return i0, i1, l0.astype(np.float64), l1.astype(np.float64)


def bilinear(src, H, W):
    """Bilinear resize to (H, W), align_corners=True."""
    x = np.asarray(src, np.float64)
    h0, h1, lh0, lh1 = axis(x.shape[2], H)
    w0, w1, lw0, lw1 = axis(x.shape[3], W)
    top = lw0 * x[:, :, h0][:, :, :, w0] + lw1 * x[:, :, h0][:, :, :, w1]
    bot = lw0 * x[:, :, h1][:, :, :, w0] + lw1 * x[:, :, h1][:, :, :, w1]
    return lh0[:, None] * top + lh1[:, None] * bot


MODES = {"copy": lambda x, H, W: copy(x), "pool": lambda x, H, W: pool2x(x), "bilinear": bilinear}


def assemble(parts, H, W):
    """parts: (mode, array) pairs; the float64 concatenation along the channels."""
    return np.concatenate([MODES[m](x, H, W) for m, x in parts], axis=1)
