"""Host side of the upsampling head (no GPU): rc_upsample_head's argument
checks with fake pointers (nothing launches), upsample.upsample_head's
refusals, and the claims of upsample_head_util's case list asserted from the
list, with the fp64 bound's cap on those inputs."""
import ctypes

import pytest
import torch

import upsample_head_util as hu
import upsample_sweep_util as usu
from raft_stereo_amd import _lib
from raft_stereo_amd.upsample import upsample_head

FAKE = 0x10000                      # 64 KiB: aligned to anything; never dereferenced on the host


def call(**kw):
    a = dict(flow=FAKE, fs=(35, 35), mask=FAKE + 0x1000, ms=None, dt=_lib.RC_BF16, scale=0.25, N=1, C=1, H=5, W=7,
             f=4, out=FAKE + 0x2000)
    a.update(kw)
    HW, MC = a["H"] * a["W"], 9 * a["f"] ** 2
    ms = a["ms"] if a["ms"] is not None else (MC * HW, HW, 1)
    return _lib.lib().rc_upsample_head(a["flow"], None if a["fs"] is None else _lib.long_array(a["fs"]), a["mask"],
                                       None if ms == "null" else _lib.long_array(ms), a["dt"], a["scale"], a["N"],
                                       a["C"], a["H"], a["W"], a["f"], a["out"], None)


@pytest.mark.parametrize("kw,code", [
    (dict(f=3), _lib.RC_EINVAL),
    (dict(f=0), _lib.RC_EINVAL),
    (dict(f=16), _lib.RC_EINVAL),
    (dict(flow=None), _lib.RC_EINVAL),
    (dict(mask=None), _lib.RC_EINVAL),
    (dict(out=None), _lib.RC_EINVAL),
    (dict(dt=3), _lib.RC_EINVAL),
    (dict(dt=-1), _lib.RC_EINVAL),
    (dict(out=FAKE + 0x2000 + 8), _lib.RC_EINVAL),            # f = 4: 16 bytes
    (dict(out=FAKE + 0x2000 + 4, f=2), _lib.RC_EINVAL),       # f = 2: 8 bytes
    (dict(mask=FAKE + 0x1001), _lib.RC_EINVAL),               # not aligned to a bf16 element
    (dict(C=0), _lib.RC_EINVAL),
    (dict(N=-1), _lib.RC_EINVAL),
    (dict(fs=None), _lib.RC_EINVAL),
    (dict(ms="null"), _lib.RC_EINVAL),
    (dict(ms=(144 * 35, 35, -1)), _lib.RC_EINVAL),
    (dict(ms=(144 * 35, 36, 1)), _lib.RC_EUNSUPPORTED),       # padded planes
    (dict(ms=(144 * 35, 35, 2)), _lib.RC_EUNSUPPORTED),       # planar with a pixel stride
    (dict(ms=(144 * 35, 1, 145)), _lib.RC_EUNSUPPORTED),      # padded channels-last pixels
    (dict(ms=(144 * 35, 2, 144)), _lib.RC_EUNSUPPORTED),
    (dict(ms=(144 * 35, 7, 5)), _lib.RC_EUNSUPPORTED),
    (dict(N=0), _lib.RC_OK),
    (dict(H=0), _lib.RC_OK),
    (dict(W=0), _lib.RC_OK),
    (dict(N=0, flow=None, mask=None, out=None), _lib.RC_OK),
])
def test_validation_codes(kw, code):
    assert call(**kw) == code
    if code:
        assert b"rc_upsample_head" in _lib.lib().rc_last_error()


def test_refusals_come_before_the_empty_problem():
    assert call(N=0, f=3) == _lib.RC_EINVAL
    assert call(N=0, dt=7) == _lib.RC_EINVAL
    assert call(N=0, ms=(0, 2, 144)) == _lib.RC_EUNSUPPORTED


def test_signature():
    res, args = _lib.SIGNATURES["rc_upsample_head"]
    assert res is ctypes.c_int and args[5] is ctypes.c_float and len(args) == 13


# ------------------------------------------------------------ python refusals

def test_python_refuses_cpu_tensors():
    with pytest.raises(RuntimeError, match="HIP"):
        upsample_head(torch.zeros(1, 1, 2, 3), torch.zeros(1, 144, 2, 3), 4)


class _OnHip:
    """Tensors that claim a HIP device: the checks in front of the launch
    look at nothing else on the host."""

    def __init__(self, monkeypatch):
        from raft_stereo_amd import upsample
        monkeypatch.setattr(upsample, "_require_hip", lambda t, what: None)


def test_python_refuses_wrong_mask_shape(monkeypatch):
    _OnHip(monkeypatch)
    with pytest.raises(RuntimeError, match="mask"):
        upsample_head(torch.zeros(1, 1, 2, 3), torch.zeros(1, 36, 2, 3), 4)
    with pytest.raises(RuntimeError, match="4-D"):
        upsample_head(torch.zeros(1, 2, 3), torch.zeros(1, 144, 2, 3), 4)


def test_python_refuses_float64(monkeypatch):
    _OnHip(monkeypatch)
    with pytest.raises(RuntimeError, match="float64"):
        upsample_head(torch.zeros(1, 1, 2, 3), torch.zeros(1, 144, 2, 3, dtype=torch.float64), 4)


def test_python_refuses_requires_grad(monkeypatch):
    _OnHip(monkeypatch)
    mask = torch.zeros(1, 144, 2, 3, requires_grad=True)
    with torch.enable_grad(), pytest.raises(RuntimeError, match=r"convex_upsample\(\.\.\., differentiable=True\)"):
        upsample_head(torch.zeros(1, 1, 2, 3), mask, 4)


# ------------------------------------------------------------------ the list

@pytest.mark.parametrize("f", hu.FACTORS)
def test_case_list_claims(f):
    cs = hu.cases(f)
    assert len(cs) == len(set(cs)) == len(hu.WIDTHS) + 3
    for W in (1, 2, 3, 21, 22, 63, 64, 65, 70):
        assert (2, 2, 3, W, f) in cs
    assert (1, 1, 1, 1, f) in cs and (3, 1, 1, 13, f) in cs and (1, 1, 1, 256 // f + 1, f) in cs
    # rows that wrap inside a wave: a row shorter than 64 pixels with a next row
    assert any(H > 1 and W < 64 for _, _, H, W, _ in cs)
    # taps in the neighbouring 64-pixel group: an image of more than 64 pixels and several rows
    assert any(H > 1 and H * W > 64 for _, _, H, W, _ in cs)
    # several images in one 64-pixel group
    assert any(N >= 3 and N * H * W <= 64 for N, _, H, W, _ in cs)
    # one lane past a 256-lane block: N H W f = 256 + f lanes of sub-rows
    assert (256 // f + 1) * f == 256 + f
    for dt in hu.DTYPES:
        # planar: the 8-byte instance where H W is a multiple of its V pixels, the narrow one elsewhere
        assert {hu.wide(c, dt, "planar") for c in cs} == {True, False}, dt
        assert any(hu.wide(c, dt, "planar") and hu.groups(c, dt, "planar") > 64 for c in cs) or dt != "f32"
        # interleaved: an aligned base always takes the vector of f elements
        assert {hu.wide(c, dt, "interleaved") for c in cs} == {True}, dt
        # the odd case, its mask one element off: the narrow instances (at f = 1 the vector is the element)
        odd = hu.ODD + (f,)
        assert not hu.wide(odd, dt, "planar", hu.es(dt))
        assert hu.wide(odd, dt, "interleaved", hu.es(dt)) == (f == 1)
    # more than one workgroup in the single-pixel-group classes
    assert any(N * H * W > 64 for N, _, H, W, _ in cs)


def test_dtypes_and_scales():
    assert set(hu.DTYPES) == {"f32", "f16", "bf16"} and hu.SCALES == (0.25, 1.0)
    assert hu.MASK_SCALES == (2.0, 40.0) and hu.FACTORS == (1, 2, 4, 8)
    # the one-hot routing logits are exact in both half formats
    for dt in (torch.float16, torch.bfloat16):
        assert float(torch.tensor(usu.OFF).to(dt)) == usu.OFF
    # the routing test passes scale 1.0: 0.25 * -200 = -50, and e^-50 is not 0 in fp32
    assert float(torch.exp(torch.tensor(-50.0))) > 0.0


@pytest.mark.parametrize("mscale", hu.MASK_SCALES)
@pytest.mark.parametrize("f", hu.FACTORS)
def test_cpu_restatement_stays_under_the_cap(f, mscale):
    """The GPU bound is max(1e-5, 4 r_cpu) with r_cpu the fp32 CPU
    restatement's error on the widened, scaled mask: on every input of the
    list 4 r_cpu stays under upsample_sweep_util.CAP."""
    worst = 0.0
    for c in hu.cases(f) + [hu.ODD + (f,)]:
        for dt in hu.DTYPES:
            for s in hu.SCALES:
                worst = max(worst, hu.reference(c, mscale, dt, s)[3])
    print(f"f = {f}, mask scale {mscale}: worst r_cpu {worst:.2e}")
    assert 4 * worst <= usu.CAP
