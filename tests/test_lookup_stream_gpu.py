"""The pair lookup's instruction stream (csrc/lookup_pair.h: the pinned load
schedule, the edge taps evaluated once, the 3-way tap selects) against the
per-level lookup on the materialised pyramid and the C oracle, value for
value (NaN == NaN), on coordinate fields that reach every case of the selects
wave by wave: all lanes with moved floors (x = w1), none (a fractional
field), one lane in 64, the fp32 neighbours of the integers (the only way to
the select's hi case) and the special values of test_corr_gpu.py.
tests/test_lookup_taps_host.py proves on the CPU what each field reaches."""
import functools

import numpy as np
import pytest
import torch

from lookup_stream_util import coords, fractional_x, integer_x, mixed_x, rows_x, special_x
from oracle import coracle
from raft_stereo_amd import CorrBlock1D
from raft_stereo_amd import corr as rcorr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

SHAPES = [
    # B, D, H, W1, W2
    (1, 32, 3, 240, 240),
    (2, 32, 2, 70, 24),      # a partial wave; level widths 24 / 12 / 6 / 3
    (1, 32, 2, 65, 17),      # level 3 has W = 2: W - 1 = 1
]
sid = lambda s: "x".join(map(str, s))  # noqa: E731


@functools.lru_cache(maxsize=None)
def fmaps(shape):
    B, D, H, W1, W2 = shape
    g = torch.Generator().manual_seed(5100 + sum(shape))
    return torch.randn(B, D, H, W1, generator=g).to(DEV), torch.randn(B, D, H, W2, generator=g).to(DEV)


@functools.lru_cache(maxsize=None)
def fields(shape):
    """name -> (B, 2, H, W1) coordinates (CPU)."""
    B, D, H, W1, W2 = shape
    dmax = min(64, W2)
    if shape == SHAPES[0]:      # one source per image row: integer, fractional, one integer lane per wave
        out = {"rows": rows_x(W1, W2, 21)}
    else:
        out = {"integer": integer_x(B, H, W1), "fractional": fractional_x(B, H, W1, 22, dmax),
               "mixed": mixed_x(B, H, W1, W2, 23, dmax)}
    out["special"] = special_x(B, H, W1, W2, 24, dmax)
    return {k: coords(v) for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def reference(shape, L, r, bf16):
    """name -> the per-level lookup over the materialised pyramid (fp32, on the
    GPU), itself checked against the C oracle once."""
    f1, f2 = fmaps(shape)
    out = {}
    with torch.no_grad():
        blk = CorrBlock1D(f1, f2, num_levels=L, radius=r, pyramid_dtype=torch.bfloat16 if bf16 else None)
        pyr = blk.corr_pyramid
        pyr_np = [t.reshape(t.shape[0], -1).float().cpu().numpy() for t in pyr]
        for name, c in fields(shape).items():
            ref = rcorr.lookup(pyr, c.to(DEV), L, r)
            np.testing.assert_array_equal(ref.cpu().numpy(), coracle.corr_lookup(pyr_np[:L], c.numpy(), L, r))
            out[name] = ref
    return out


def check(got, ref, what):
    np.testing.assert_array_equal(got.float().cpu().numpy(), ref.float().cpu().numpy(), err_msg=what)


VARIANTS = {
    "nl4_r4": dict(L=4, r=4),
    "nl2_r4": dict(L=2, r=4),
    "nl4_r1": dict(L=4, r=1),
    "nl2_r1": dict(L=2, r=1),
    "bf16_nl4_r4": dict(L=4, r=4, bf16=True),
    "bf16_nl2_r1": dict(L=2, r=1, bf16=True),
    "shadow2": dict(L=4, r=4, kw=dict(shadow=(2,))),
    "out_f16": dict(L=4, r=4, kw=dict(out_dtype=torch.float16)),
    "channels_last": dict(L=4, r=4, kw=dict(channels_last=True)),
    "bf16_channels_last_f16": dict(L=4, r=4, bf16=True, kw=dict(channels_last=True, out_dtype=torch.float16)),
}


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_pair_lookup_matches_per_level_and_oracle(shape, variant):
    v = VARIANTS[variant]
    L, r, bf16, kw = v["L"], v["r"], v.get("bf16", False), v.get("kw", {})
    f1, f2 = fmaps(shape)
    ref = reference(shape, L, r, bf16)
    with torch.no_grad():
        blk = CorrBlock1D(f1, f2, num_levels=L, radius=r, pyramid_dtype=torch.bfloat16 if bf16 else None, **kw)
        assert blk._chain and blk.levels_stored == ([0, 2] if L == 4 else [0])
        if "shadow" in kw:
            assert blk._shadow
        for name, c in fields(shape).items():
            got = blk(c.to(DEV))
            want = ref[name].to(kw["out_dtype"]) if "out_dtype" in kw else ref[name]
            assert got.dtype == want.dtype and got.shape == want.shape
            if kw.get("channels_last"):
                assert got.is_contiguous(memory_format=torch.channels_last)
            check(got, want, f"{variant} {name}")


@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_lookup_step_matches(shape):
    """The fused loop step runs the same pair kernel (first iteration: no delta)."""
    f1, f2 = fmaps(shape)
    ref = reference(shape, 4, 4, False)
    with torch.no_grad():
        blk = CorrBlock1D(f1, f2, num_levels=4, radius=4)
        for name, c in fields(shape).items():
            corr, new, _ = blk.lookup_step(c.to(DEV))
            assert torch.equal(new.cpu().view(torch.int32), c.view(torch.int32))
            check(corr, ref[name], f"step {name}")


def test_disparity_layout_matches():
    """layout="disparity": the sheared pair kernel shares plan_pair / finish_pair."""
    shape = SHAPES[0]
    f1, f2 = fmaps(shape)
    ref = reference(shape, 4, 4, False)
    with torch.no_grad():
        blk = CorrBlock1D(f1, f2, num_levels=4, radius=4, layout="disparity")
        assert blk.layout == "disparity"
        for name, c in fields(shape).items():
            check(blk(c.to(DEV)), ref[name], f"disparity {name}")


def test_records_layout_matches():
    """layout="records" (bf16, D = 256): the records kernel shares plan_pair /
    finish_pair; its reference is the per-level lookup over its own pyramid."""
    B, D, H, W1, W2 = 1, 256, 3, 240, 240
    g = torch.Generator().manual_seed(5200)
    f1 = torch.randn(B, D, H, W1, generator=g).to(DEV, torch.bfloat16)
    f2 = torch.randn(B, D, H, W2, generator=g).to(DEV, torch.bfloat16)
    with torch.no_grad():
        blk = CorrBlock1D(f1, f2, num_levels=4, radius=4, layout="records")
        assert blk.layout == "records"
        pyr = blk.corr_pyramid
        pyr_np = [t.reshape(t.shape[0], -1).float().cpu().numpy() for t in pyr]
        for name, c in fields(SHAPES[0]).items():
            got = blk(c.to(DEV))
            check(got, rcorr.lookup(pyr, c.to(DEV), 4, 4), f"records {name}")
            np.testing.assert_array_equal(got.cpu().numpy(), coracle.corr_lookup(pyr_np[:4], c.numpy(), 4, 4))
