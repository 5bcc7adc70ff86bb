"""RC_OUT_F16 / RC_OUT_BF16 (ABI v13): the flags' values,
where the C-ABI accepts them (the pair and records kernels behind
rc_corr_lookup_chain / rc_corr_lookup_step) and where it refuses them, all
before any launch -- no GPU needed (B = 0 with fake pointers, as in
test_capi.py) -- and the Python option's argument check."""
import ctypes
import re

import pytest
import torch

import raft_stereo_amd  # noqa: F401  (registered by conftest)
from raft_stereo_amd import CorrBlock1D, _lib

FLAGS = [("RC_OUT_F16", "f16"), ("RC_OUT_BF16", "bf16")]


def f(a):
    return ctypes.c_void_p(a)


def test_flag_values_and_abi_version():
    text = open(_lib.HEADER).read()
    for name, _ in FLAGS:
        m = re.search(rf"#define {name}\s+(0x[0-9a-fA-F]+)", text)
        assert m and int(m.group(1), 16) == getattr(_lib, name), name
    assert _lib.RC_OUT_F16 != _lib.RC_OUT_BF16
    # bits of their own: no other pyr_dtype flag, and 0x400000 stays unknown
    others = (0xFF | _lib.RC_SHADOW | _lib.RC_OUT_CHANNELS_LAST | _lib.RC_BUILD_EXACT_F32
              | _lib.RC_LAYOUT_DISPARITY | _lib.RC_LAYOUT_RECORDS | 0x400000)
    assert (_lib.RC_OUT_F16 | _lib.RC_OUT_BF16) & others == 0
    assert _lib.lib().rc_abi_version() == _lib.ABI_VERSION == 13


def _chain(dt, ptrs=None, w=None, levels=2, B=0):
    ptrs = _lib.ptr_array([f(0x1000), None]) if ptrs is None else ptrs
    w = _lib.int_array([64, 32]) if w is None else w
    return _lib.lib().rc_corr_lookup_chain(ptrs, w, None, dt, levels, 4, f(0x2000), 0, B, 1, 64, f(0x3000), None)


def _step(dt, chain, ptrs=None, w=None, levels=2, B=0):
    ptrs = _lib.ptr_array([f(0x1000), None]) if ptrs is None else ptrs
    w = _lib.int_array([64, 32]) if w is None else w
    return _lib.lib().rc_corr_lookup_step(ptrs, w, None, dt, levels, 4, chain, f(0x2000), None, f(0x3000),
                                          f(0x5000), B, 1, 64, f(0x4000), None)


@pytest.mark.parametrize("name", [n for n, _ in FLAGS])
def test_flag_accepted_by_pair_and_records(name):
    """Each flag alone passes every check of the two entry points the pair /
    records kernels serve (B = 0: RC_OK after the checks, nothing launched),
    with and without RC_OUT_CHANNELS_LAST and shadow copies."""
    flag = getattr(_lib, name)
    for extra in (0, _lib.RC_OUT_CHANNELS_LAST, _lib.RC_SHADOW, _lib.RC_OUT_CHANNELS_LAST | _lib.shadow_level(0)):
        assert _chain(_lib.RC_F32 | flag | extra) == _lib.RC_OK
        assert _step(_lib.RC_F32 | flag | extra, 1) == _lib.RC_OK
        assert _chain(_lib.RC_BF16 | flag | extra) == _lib.RC_OK
    four = _lib.ptr_array([f(0x1000), None, f(0x2000), None])
    w4 = _lib.int_array([64, 32, 16, 8])
    assert _chain(_lib.RC_F32 | flag, four, w4, 4) == _lib.RC_OK
    assert _step(_lib.RC_BF16 | flag, 1, four, w4, 4) == _lib.RC_OK
    rec = _lib.ptr_array([f(0x1000), None, None, None])
    w4r = _lib.int_array([128, 64, 32, 16])
    for extra in (0, _lib.RC_OUT_CHANNELS_LAST):
        dt = _lib.RC_BF16 | _lib.RC_LAYOUT_RECORDS | flag | extra
        assert _chain(dt, rec, w4r, 4) == _lib.RC_OK
        assert _step(dt, 1, rec, w4r, 4) == _lib.RC_OK


def test_both_flags_are_invalid():
    L = _lib.lib()
    both = _lib.RC_F32 | _lib.RC_OUT_F16 | _lib.RC_OUT_BF16
    assert _chain(both) == _lib.RC_EINVAL and L.rc_last_error()
    assert _step(both, 1) == _lib.RC_EINVAL and L.rc_last_error()


@pytest.mark.parametrize("name", [n for n, _ in FLAGS])
def test_flag_refused_elsewhere(name):
    """RC_EUNSUPPORTED, with a message, wherever another kernel would serve
    the call: every other entry point with a pyr_dtype, the step's per-level
    lookup (chain = 0), the disparity-major layout, the level-1 chain."""
    L = _lib.lib()
    dt = _lib.RC_F32 | getattr(_lib, name)
    one = _lib.ptr_array([f(0x1000)])
    w1 = _lib.int_array([8])

    def refused(rc):
        assert rc == _lib.RC_EUNSUPPORTED
        assert L.rc_last_error()

    refused(L.rc_corr_lookup(one, w1, None, dt, 1, 4, f(0x2000), 0, 0, 1, 8, f(0x3000), None))
    refused(L.rc_corr_lookup_conv(one, w1, None, dt, 1, 4, f(0x2000), 0, 0, 1, 8, f(0x4000), None, 4, 1,
                                  f(0x3000), None))
    refused(L.rc_corr_build(None, None, 0, 0, 8, 1, 8, 8, _lib.ptr_array([None]), None, 1, dt, None))
    refused(L.rc_corr_pool(None, 8, None, 4, 0, 8, dt, None))
    refused(_step(dt, 0))
    refused(_step(dt, 0, B=1))
    refused(_chain(dt | _lib.RC_LAYOUT_DISPARITY))
    three = _lib.ptr_array([f(0x1000), f(0x2000), None])
    w3 = _lib.int_array([64, 32, 16])
    refused(_chain(dt, three, w3, 3))
    refused(_step(dt, 1, three, w3, 3))
    refused(_chain(dt, three, w3, 3, B=1))
    # 4 levels without level 2: the level-1 chain as well
    four = _lib.ptr_array([f(0x1000), f(0x2000), None, None])
    refused(_chain(dt, four, _lib.int_array([64, 32, 16, 8]), 4))


def test_python_option_checks_its_argument_before_the_build():
    """out_dtype is validated first: a bad value raises ValueError even for
    CPU tensors, which the build itself would refuse with a RuntimeError."""
    z = torch.zeros(1, 8, 1, 16)
    with pytest.raises(ValueError, match="out_dtype"):
        CorrBlock1D(z, z, out_dtype=torch.float64)
    with pytest.raises(ValueError, match="out_dtype"):
        CorrBlock1D(z, z, out_dtype="half")
    for ok in (None, torch.float32, torch.float16, torch.bfloat16):
        with pytest.raises(RuntimeError):          # past the option: "no CPU fallback"
            CorrBlock1D(z, z, out_dtype=ok)


def test_network_option_checks_its_argument():
    from raft_stereo_amd.network import RAFTStereo, StereoArgs
    with pytest.raises(ValueError, match="corr_out_dtype"):
        RAFTStereo(StereoArgs(), corr_out_dtype="fp16")
    # the keyword reaches the corr block only when the option is set
    assert RAFTStereo(StereoArgs())._corr_kwargs() == {}
    assert RAFTStereo(StereoArgs(), corr_out_dtype=torch.bfloat16)._corr_kwargs() == {"out_dtype": torch.bfloat16}
    assert RAFTStereo(StereoArgs(mixed_precision=False), corr_out_dtype="autocast")._corr_kwargs() == {}
