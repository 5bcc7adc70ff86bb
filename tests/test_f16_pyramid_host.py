"""RC_F16, the fp16 pyramid element type: its value, where
the C-ABI accepts it (rc_corr_build, rc_corr_pool, rc_corr_lookup and the pair
layout of rc_corr_lookup_chain) and where it refuses it, all before any launch
-- no GPU needed (B = 0 with fake pointers, as in test_out_dtype_host.py) --
and the argument checks of the Python options."""
import ctypes
import re

import pytest
import torch

import raft_stereo_amd  # noqa: F401  (registered by conftest)
from raft_stereo_amd import CorrBlock1D, _lib

F16, BF16, F32 = _lib.RC_F16, _lib.RC_BF16, _lib.RC_F32


def f(a):
    return ctypes.c_void_p(a)


def refused(rc):
    assert rc == _lib.RC_EUNSUPPORTED, rc
    assert _lib.lib().rc_last_error()


def test_value_matches_header_and_abi_version_stays():
    text = open(_lib.HEADER).read()
    m = re.search(r"#define RC_F16\s+(\d+)", text)
    assert m and int(m.group(1)) == _lib.RC_F16 == 2
    assert len({_lib.RC_F32, _lib.RC_BF16, _lib.RC_F16}) == 3
    assert _lib.lib().rc_abi_version() == _lib.ABI_VERSION == 13
    assert re.search(r"#define RC_ABI_VERSION\s+13\b", text)


def _build(fmap_dt, pyr_dt, nbuf=3, ptrs=None, B=0, W=64):
    ptrs = _lib.ptr_array([f(0x1000), f(0x2000), f(0x3000)][:nbuf]) if ptrs is None else ptrs
    return _lib.lib().rc_corr_build(f(0x10000), f(0x20000), fmap_dt, B, 256, 1, W, W, ptrs, None, nbuf, pyr_dt,
                                    None)


def test_build_accepts_f16_pyramid_from_f16_and_f32_fmaps():
    for fmap_dt in (F16, F32):
        assert _build(fmap_dt, F16) == _lib.RC_OK
        # RC_SHADOW_LEVEL bits as for bf16, and the pair layout (level 1 not stored)
        assert _build(fmap_dt, F16 | _lib.shadow_level(0) | _lib.shadow_level(2)) == _lib.RC_OK
        assert _build(fmap_dt, F16 | _lib.RC_SHADOW) == _lib.RC_OK
        pair = _lib.ptr_array([f(0x1000), None, f(0x3000)])
        assert _build(fmap_dt, F16 | _lib.shadow_level(2), ptrs=pair) == _lib.RC_OK
    # what was accepted before still is
    assert _build(BF16, BF16) == _lib.RC_OK and _build(F32, BF16) == _lib.RC_OK
    assert _build(F32, F32) == _lib.RC_OK and _build(BF16, F32) == _lib.RC_OK


@pytest.mark.parametrize("B", [0, 1])
def test_build_refusals(B):
    """Each refusal of rc_corr_build, whatever the size (B = 1 would launch
    on the fake pointers if a check were missing)."""
    refused(_build(F16, F32, B=B))                                   # (RC_F16, RC_F32)
    refused(_build(F16, BF16, B=B))                                  # every fp16 / bf16 mix
    refused(_build(BF16, F16, B=B))
    rec = _lib.ptr_array([f(0x1000), None, None])
    refused(_build(F16, F16 | _lib.RC_LAYOUT_RECORDS, ptrs=rec, B=B, W=128))
    refused(_build(F32, F16 | _lib.RC_LAYOUT_RECORDS, ptrs=rec, B=B, W=128))
    pair = _lib.ptr_array([f(0x1000), None, f(0x3000)])
    refused(_build(F16, F16 | _lib.RC_LAYOUT_DISPARITY, ptrs=pair, B=B))
    refused(_build(F32, F16 | _lib.RC_LAYOUT_DISPARITY, ptrs=pair, B=B))
    refused(_build(F16, F16 | _lib.RC_BUILD_EXACT_F32, B=B))
    refused(_build(F32, F16 | _lib.RC_BUILD_EXACT_F32, B=B))
    # an unknown element type stays invalid, not "unsupported"
    assert _build(3, F16, B=B) == _lib.RC_EINVAL
    assert _build(F16, 3, B=B) == _lib.RC_EINVAL


def test_pool_and_per_level_lookup_accept_f16():
    L = _lib.lib()
    assert L.rc_corr_pool(None, 8, None, 4, 0, 8, F16, None) == _lib.RC_OK
    assert L.rc_corr_pool(None, 8, None, 4, 0, 8, 3, None) == _lib.RC_EINVAL
    for levels in (1, 3, 4):
        ptrs = _lib.ptr_array([f(0x1000 * (i + 1)) for i in range(levels)])
        w = _lib.int_array([64 >> i for i in range(levels)])
        for r in (1, 4, 8):
            assert L.rc_corr_lookup(ptrs, w, None, F16, levels, r, f(0x9000), 0, 0, 1, 64, f(0xA000),
                                    None) == _lib.RC_OK


def _chain(dt, ptrs=None, w=None, levels=2, B=0):
    ptrs = _lib.ptr_array([f(0x1000), None]) if ptrs is None else ptrs
    w = _lib.int_array([64, 32]) if w is None else w
    return _lib.lib().rc_corr_lookup_chain(ptrs, w, None, dt, levels, 4, f(0x2000), 0, B, 1, 64, f(0x3000), None)


def test_chain_accepts_f16_on_the_pair_layout_only():
    four = _lib.ptr_array([f(0x1000), None, f(0x2000), None])
    w4 = _lib.int_array([64, 32, 16, 8])
    for extra in (0, _lib.RC_SHADOW, _lib.RC_OUT_CHANNELS_LAST, _lib.RC_OUT_F16, _lib.RC_OUT_BF16,
                  _lib.RC_OUT_CHANNELS_LAST | _lib.RC_OUT_F16 | _lib.shadow_level(0)):
        assert _chain(F16 | extra) == _lib.RC_OK
        assert _chain(F16 | extra, four, w4, 4) == _lib.RC_OK
    # as for bf16: the level-1 chain (3 levels, or 4 without level 2) reads fp32 only
    three = _lib.ptr_array([f(0x1000), f(0x2000), None])
    w3 = _lib.int_array([64, 32, 16])
    for B in (0, 1):
        refused(_chain(F16, three, w3, 3, B=B))
        refused(_chain(F16, _lib.ptr_array([f(0x1000), f(0x2000), None, None]), w4, 4, B=B))
        # records and disparity-major levels hold bf16 / fp32
        refused(_chain(F16 | _lib.RC_LAYOUT_RECORDS, _lib.ptr_array([f(0x1000), None, None, None]),
                       _lib.int_array([128, 64, 32, 16]), 4, B=B))
    refused(_chain(F16 | _lib.RC_LAYOUT_DISPARITY, four, w4, 4))
    assert _chain(F16 | _lib.RC_OUT_F16 | _lib.RC_OUT_BF16) == _lib.RC_EINVAL


@pytest.mark.parametrize("B", [0, 1])
def test_every_other_entry_point_refuses_f16(B):
    """RC_EUNSUPPORTED with a message, before any launch (B = 1 included):
    the fused step, the fused convc1 kernels on either layout, and their
    backwards."""
    L = _lib.lib()
    two = _lib.ptr_array([f(0x1000), None])
    full = _lib.ptr_array([f(0x1000), f(0x2000)])
    w2 = _lib.int_array([64, 32])
    for chain in (0, 1):
        for dt in (F16, F16 | _lib.RC_OUT_F16, F16 | _lib.RC_LAYOUT_RECORDS):
            if chain == 0 and dt != F16:
                continue                                   # refused for the flag itself
            refused(L.rc_corr_lookup_step(two if chain else full, w2, None, dt, 2, 4, chain, f(0x2000), None,
                                          f(0x3000), f(0x5000), B, 1, 64, f(0x4000), None))
    refused(L.rc_corr_lookup_conv(full, w2, None, F16, 2, 4, f(0x2000), 0, B, 1, 64, f(0x4000), None, 4, 1,
                                  f(0x3000), None))
    refused(L.rc_corr_lookup_conv_backward(full, w2, None, F16, 2, 4, f(0x2000), 0, B, 1, 64, f(0x4000), None, 4,
                                           1, f(0x5000), f(0x6000), None, None, None, None))
    refused(L.rc_corr_lookup_chain_conv(two, w2, None, F16, 2, 4, f(0x2000), 0, B, 1, 64, f(0x4000), None, 4, 1,
                                        f(0x3000), None))
    refused(L.rc_corr_lookup_chain_conv(two, w2, None, F16 | _lib.RC_OUT_F16, 2, 4, f(0x2000), 0, B, 1, 64,
                                        f(0x4000), None, 4, 1, f(0x3000), None))
    refused(L.rc_corr_lookup_chain_conv_backward(two, w2, None, F16, 2, 4, f(0x2000), 0, B, 1, 64, f(0x4000), None,
                                                 4, 1, f(0x5000), f(0x6000), None, None, None, None))
    # rc_corr_build_backward is unchanged: fp32 fmaps only
    refused(L.rc_corr_build_backward(f(0x1000), f(0x2000), F16, B, 8, 1, 64, 64, _lib.ptr_array([f(0x3000)]), None,
                                     1, f(0x4000), f(0x5000), None))


def test_python_option_reaches_the_build():
    """pyramid_dtype=torch.float16 is an accepted option now: CPU tensors get
    the build's "no CPU fallback" RuntimeError, not a TypeError for the dtype."""
    z = torch.zeros(1, 8, 1, 16)
    for fm in (z, z.half()):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            CorrBlock1D(fm, fm, pyramid_dtype=torch.float16)
    from raft_stereo_amd import corr as rcorr
    assert rcorr._dtype_code(torch.float16) == _lib.RC_F16
    assert rcorr.shadow_fits(1000, 311, torch.float16) == rcorr.shadow_fits(1000, 311, torch.bfloat16)
    # the defaults follow the element size: fp16 as bf16
    big = 64 * 94 * 311
    assert (rcorr.default_shadow_levels(big, 311, 4, torch.float16)
            == rcorr.default_shadow_levels(big, 311, 4, torch.bfloat16) == (0, 2))
    assert rcorr.default_shadow_levels(1000, 311, 4, torch.float16) == (2,)


def test_python_option_refusals_need_no_device():
    z = torch.zeros(1, 8, 1, 16)
    with pytest.raises(ValueError, match="bfloat16"):
        CorrBlock1D(z.bfloat16(), z.bfloat16(), pyramid_dtype=torch.float16)
    with pytest.raises(ValueError, match="bfloat16"):
        CorrBlock1D(z, z.bfloat16(), pyramid_dtype=torch.float16)
    for layout in ("records", "disparity"):
        with pytest.raises(ValueError, match=layout):
            CorrBlock1D(z, z, pyramid_dtype=torch.float16, layout=layout)
    with pytest.raises(ValueError, match="exact_f32"):
        CorrBlock1D(z, z, pyramid_dtype=torch.float16, exact_f32=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):      # "auto" resolves to rows
        CorrBlock1D(z, z, pyramid_dtype=torch.float16, layout="auto")


def test_network_option_checks_its_argument():
    from raft_stereo_amd.network import RAFTStereo, StereoArgs
    with pytest.raises(ValueError, match="corr_pyramid_dtype"):
        RAFTStereo(StereoArgs(), corr_pyramid_dtype="fp16")
    with pytest.raises(ValueError, match="corr_pyramid_dtype"):
        RAFTStereo(StereoArgs(), corr_pyramid_dtype=16)
    # the keyword reaches the corr block only when the option is set
    assert RAFTStereo(StereoArgs())._corr_kwargs() == {}
    assert (RAFTStereo(StereoArgs(), corr_pyramid_dtype=torch.float16)._corr_kwargs()
            == {"pyramid_dtype": torch.float16})
    assert (RAFTStereo(StereoArgs(), corr_pyramid_dtype=torch.float16, corr_out_dtype=torch.bfloat16)._corr_kwargs()
            == {"out_dtype": torch.bfloat16, "pyramid_dtype": torch.float16})
    # "autocast" without mixed precision: nothing
    assert RAFTStereo(StereoArgs(mixed_precision=False), corr_pyramid_dtype="autocast")._corr_kwargs() == {}
    mp = RAFTStereo(StereoArgs(mixed_precision=True), corr_pyramid_dtype="autocast")._corr_kwargs()
    assert mp == ({"pyramid_dtype": torch.float16} if torch.cuda.is_available() else {})
