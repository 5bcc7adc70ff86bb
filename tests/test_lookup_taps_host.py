"""Which cases of the pair lookup's 3-way tap select (csrc/lookup_pair.h,
window_taps: x0 below, at or above the nominal n_t) the coordinate fields of
tests/test_lookup_stream_gpu.py reach, proved on the CPU with a numpy
restatement of one tap's fp32 op sequence (lookup_stream_util.tap_floors).
No GPU."""
import numpy as np

from lookup_stream_util import fractional_x, integer_x, mixed_x, moved_lanes, moved_taps, nextafter_x

W2, L, R = 240, 4, 4


def test_integer_coordinates_move_floors_at_every_level():
    """x = w1 (the network's first iteration): at every level some tap's
    floor lands one below its nominal n_t (the select's lo case), never above."""
    x = integer_x(1, 1, W2).numpy().reshape(-1)
    moved = moved_taps(x, W2, L, R)
    print("taps with x0 < nt, x0 > nt per level:", moved, "of", W2 * (2 * R + 1))
    assert [m[0] for m in moved] == [227, 255, 57, 24]
    assert all(lo >= 1 and hi == 0 for lo, hi in moved)


def test_fractional_field_moves_no_floor():
    """The seeded fractional fields of the GPU test: no tap leaves its nominal
    position at any level: every select takes its middle case."""
    for shape, dmax in (((1, 1, 240), 64), ((2, 2, 70), 24), ((1, 2, 65), 17)):
        x = fractional_x(*shape, seed=11, dmax=dmax).numpy().reshape(-1)
        for W in (240, 24, 17):
            assert moved_taps(x, W, L, R) == [(0, 0)] * L, (shape, W)
            assert moved_taps(x, W, 2, 1) == [(0, 0)] * 2, (shape, W)


def test_mixed_field_has_one_moved_lane_per_wave():
    """One chosen integer pixel per 64: each 64-pixel wave of the row holds
    exactly one lane with a moved floor at level 0 or 1; every other lane keeps
    all of its floors at every level."""
    for W1, Wl, dmax, r in ((240, 240, 64, 4), (70, 24, 24, 4), (65, 17, 17, 4), (240, 240, 64, 1)):
        x = mixed_x(1, 1, W1, Wl, seed=12, dmax=dmax, radius=r).numpy().reshape(-1)
        assert set(np.flatnonzero(moved_lanes(x, Wl, r))) == set(range(17, W1, 64)), (W1, Wl)
        rest = np.delete(x, np.arange(17, W1, 64))
        assert moved_taps(rest, Wl, L if r == 4 else 2, r) == [(0, 0)] * (L if r == 4 else 2)


def test_nextafter_coordinates_reach_the_hi_case():
    """x = nextafter(k, -inf): x_t rounds up to an integer whose round trip
    does not come back below it, so x0 = n_t + 1 -- the select's hi case --
    occurs at every level; x = nextafter(k, +inf) gives only the lo case.
    These coordinates therefore join the GPU test."""
    na = nextafter_x(W2)
    below, above = moved_taps(na[:W2], W2, L, R), moved_taps(na[W2:], W2, L, R)
    print("below:", below, "above:", above)
    assert all(hi >= 1 for _, hi in below)
    assert all(lo >= 1 and hi == 0 for lo, hi in above)
