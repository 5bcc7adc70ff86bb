"""float64 numpy evaluation of the ConvGRU glue (rc_gru_gates, rc_gru_blend):
the reference of tests/test_gru_gates_gpu.py.  Inputs are widened to float64;
sigmoid is evaluated in the form that does not overflow on either side."""
import numpy as np


def _f64(*arrays):
    return [np.asarray(a, np.float64) for a in arrays]


def sigmoid(a):
    a = np.asarray(a, np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.exp(-np.abs(a))
        return np.where(a >= 0, 1.0 / (1.0 + e), e / (1.0 + e))     # NaN: e is NaN, both branches are


def gates(z_pre, r_pre, cz, cr, h):
    """(z, r*h) with z = sigmoid(z_pre + cz), r = sigmoid(r_pre + cr)."""
    z_pre, r_pre, cz, cr, h = _f64(z_pre, r_pre, cz, cr, h)
    return sigmoid(z_pre + cz), sigmoid(r_pre + cr) * h


def blend(z, q_pre, cq, h):
    """(1 - z) * h + z * tanh(q_pre + cq)."""
    z, q_pre, cq, h = _f64(z, q_pre, cq, h)
    return (1.0 - z) * h + z * np.tanh(q_pre + cq)
