"""float64 numpy evaluation of the six gradients of the ConvGRU glue
(rc_gru_gates_backward, rc_gru_blend_backward): the reference of
tests/test_gru_backward_gpu.py.  Inputs are widened to float64; r comes from
gru_ref's sigmoid, the form that does not overflow on either side."""
import numpy as np

from gru_ref import _f64, sigmoid


def blend_backward(g_out, z, q_pre, cq, h):
    """(g_z, g_qpre, g_h) of h_out = (1 - z) * h + z * tanh(q_pre + cq);
    g_qpre is the gradient of cq as well."""
    g_out, z, q_pre, cq, h = _f64(g_out, z, q_pre, cq, h)
    q = np.tanh(q_pre + cq)
    return g_out * (q - h), g_out * z * (1.0 - q * q), g_out * (1.0 - z)


def gates_backward(g_z, g_rh, z, r_pre, cr, h):
    """(g_zpre, g_rpre, g_h) of z = sigmoid(z_pre + cz) and rh = sigmoid(r_pre +
    cr) * h, given z; g_zpre and g_rpre are the gradients of cz and cr as
    well."""
    g_z, g_rh, z, r_pre, cr, h = _f64(g_z, g_rh, z, r_pre, cr, h)
    r = sigmoid(r_pre + cr)
    return g_z * (1.0 - z) * z, g_rh * h * (1.0 - r) * r, g_rh * r
