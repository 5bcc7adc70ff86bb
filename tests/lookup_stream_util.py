"""Coordinate fields for the pair lookup's 3-way tap select (csrc/lookup_pair.h,
window_taps): a tap whose floor x0 keeps its nominal n_t reads window
elements t+1, t+2; one whose floor moved by one reads t, t+1 or t+2, t+3.
tests/test_lookup_taps_host.py proves on the CPU which cases each field
reaches (all lanes of a wave, none, or one lane in 64);
tests/test_lookup_stream_gpu.py runs them on the kernels.

tap_floors is a numpy restatement of one tap's fp32 op sequence
(oracle/torch_ref.py, window_taps): x_l = x / 2^i, x_t = k + x_l,
xn = RN(2 x_t / (W - 1)) - 1, x' = (xn + 1) * ((W - 1) / 2), x0 = floor(x'),
n_t = floor(x_l) + k.
"""
import numpy as np
import torch

F = np.float32


def tap_floors(x, W, level, radius):
    """(x0, nt), each [len(x), 2 radius + 1] fp32, of the taps of one level."""
    x = np.asarray(x, F).reshape(-1)
    xl = (x / F(1 << level)).astype(F)
    wm1 = F(W - 1)
    half = F(wm1 / F(2))
    k = np.arange(-radius, radius + 1, dtype=F)[None, :]
    xt = (k + xl[:, None]).astype(F)
    q = ((F(2) * xt).astype(F) / wm1).astype(F)          # IEEE division: correctly rounded, as div_rn
    xn = (q - F(1)).astype(F)
    xp = ((xn + F(1)).astype(F) * half).astype(F)
    return np.floor(xp), np.floor(xl)[:, None] + k


def moved_taps(x, W2, levels, radius):
    """Per level (lo, hi): the number of taps with x0 < n_t and with x0 > n_t."""
    out = []
    for i in range(levels):
        x0, nt = tap_floors(x, W2 >> i, i, radius)
        out.append((int((x0 < nt).sum()), int((x0 > nt).sum())))
    return out


def moved_lanes(x, W2, radius):
    """Per coordinate: some tap of level 0 or 1 leaves its nominal floor."""
    m = np.zeros(np.asarray(x).size, bool)
    for i in range(2):
        x0, nt = tap_floors(x, W2 >> i, i, radius)
        m |= (x0 != nt).any(axis=1)
    return m


def _xy(x):
    return torch.cat([x, torch.zeros_like(x)], 1)


def integer_x(B, H, W1):
    """x = w1 exactly (coords_grid: the network's first iteration)."""
    return torch.arange(W1).float().view(1, 1, 1, W1).expand(B, 1, H, W1).contiguous()


def fractional_x(B, H, W1, seed, dmax=64):
    """x = w1 - d, d an integer in [0, dmax) plus a fraction in [1/8, 7/8]: x / 2^i
    stays at least 1/64 from every integer for i <= 3, far more than the
    round trip's error (< 1e-3 at these widths), so no tap's floor moves."""
    g = torch.Generator().manual_seed(seed)
    d = torch.randint(0, dmax, (B, 1, H, W1), generator=g).float()
    d = d + 0.125 + 0.75 * torch.rand(B, 1, H, W1, generator=g)
    return integer_x(B, H, W1) - d


def mixed_x(B, H, W1, W2, seed, dmax=64, radius=4):
    """The fractional field with one exact-integer pixel per 64, an integer at
    which a tap's floor moves at level 0 or 1 (not every integer does; none
    at level 0 when W2 - 1 is a power of two): one lane that needs the selects
    in an otherwise undisturbed wave."""
    x = fractional_x(B, H, W1, seed, dmax)
    k = np.arange(W2, dtype=F)
    cand = torch.from_numpy(k[moved_lanes(k, W2, radius)])
    assert cand.numel() > 0
    sub = x[..., 17::64]
    idx = (sub.unsqueeze(-1) - cand).abs().argmin(-1)
    x[..., 17::64] = cand[idx]
    return x


def nextafter_x(W2):
    """The fp32 neighbours of every integer of the row, below then above."""
    k = np.arange(W2, dtype=F)
    return np.concatenate([np.nextafter(k, F(-np.inf)), np.nextafter(k, F(np.inf))]).astype(F)


def special_x(B, H, W1, W2, seed, dmax=64):
    """The special values of tests/test_corr_gpu.py (NaN, +-inf, +-1e30, +-0,
    subnormals, far outside the row) and the nextafter coordinates, in a
    fractional field."""
    x = fractional_x(B, H, W1, seed, dmax)
    flat = x.reshape(-1)
    vals = [float("nan"), float("inf"), -float("inf"), 1e30, -1e30, 0.0, -0.0, 1e-45, -1e-45,
            -2.8e-45, 3.0e-39, -3.0e-39, -1e-40, W2 - 1.0, W2 + 3.999, -4.5, -33.0, -35.0,
            5.0 * W2, -5.0 * W2, 1e6, -1e6]
    na = torch.from_numpy(nextafter_x(W2))
    n = min(flat.numel() - len(vals), na.numel())
    step = max(1, na.numel() // n)
    flat[:len(vals)] = torch.tensor(vals)
    flat[len(vals):len(vals) + len(na[::step][:n])] = na[::step][:n]
    return flat.view(B, 1, H, W1)


def rows_x(W1, W2, seed):
    """(1, 1, 3, W1): row 0 integer, row 1 fractional, row 2 mixed."""
    return torch.cat([integer_x(1, 1, W1), fractional_x(1, 1, W1, seed), mixed_x(1, 1, W1, W2, seed + 1)], 2)


def coords(x):
    return _xy(x)
