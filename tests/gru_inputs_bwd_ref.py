"""float64 numpy adjoint of the three modes of rc_gru_assemble (copy, pool2x,
bilinear): the reference of tests/test_gru_inputs_backward_gpu.py.  Each is
the forward of gru_inputs_ref.py transposed, built by scatter (``np.add.at``):
every destination pixel adds its gradient, times the weight the forward gave
the tap, onto the source pixel the tap read.

The bilinear weights are gru_inputs_ref.axis's: fp32 coordinates widened, as
the kernel computes them.  fp64 torch autograd is not used: its coordinates
are fp64 and differ from the kernel by the coordinates' rounding (3.5e-7
norm_err from this reference on the test's shapes; an fp32 fixed-order
evaluation is within 1.1e-7 of it)."""
import numpy as np

from gru_inputs_ref import axis


def copy(G, h, w):
    return np.asarray(G, np.float64)


def pool2x(G, h, w):
    """The adjoint of the 3x3 average, stride 2, zero padding 1 (padding
    counted) from an (h, w) source: G / 9 onto every in-image tap."""
    G = np.asarray(G, np.float64)
    N, C, H, W = G.shape
    assert (H, W) == ((h - 1) // 2 + 1, (w - 1) // 2 + 1)
    out = np.zeros((N, C, h, w))
    oy, ox = np.arange(H), np.arange(W)
    for kh in range(3):
        ih = 2 * oy - 1 + kh
        my = (ih >= 0) & (ih < h)
        for kw in range(3):
            iw = 2 * ox - 1 + kw
            mx = (iw >= 0) & (iw < w)
            np.add.at(out, (slice(None), slice(None), ih[my][:, None], iw[mx][None, :]),
                      G[:, :, my][:, :, :, mx] / 9.0)
    return out


def bilinear(G, h, w):
    """The adjoint of the bilinear resize (align_corners=True) from an (h, w)
    source to G's size: the four taps' weights times G, scattered."""
    G = np.asarray(G, np.float64)
    N, C, H, W = G.shape
    h0, h1, lh0, lh1 = axis(h, H)
    w0, w1, lw0, lw1 = axis(w, W)
    out = np.zeros((N, C, h, w))
    for ih, lh in ((h0, lh0), (h1, lh1)):
        for iw, lw in ((w0, lw0), (w1, lw1)):
            np.add.at(out, (slice(None), slice(None), ih[:, None], iw[None, :]), lh[:, None] * lw[None, :] * G)
    return out


MODES = {"copy": copy, "pool": pool2x, "bilinear": bilinear}


def assemble_backward(G, parts):
    """G: the (N, sum C, H, W) gradient; parts: (mode, C, h, w) each.  The
    float64 gradient of every part's source, in order."""
    outs, c = [], 0
    for mode, C, h, w in parts:
        outs.append(MODES[mode](G[:, c:c + C], h, w))
        c += C
    return outs
