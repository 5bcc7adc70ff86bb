"""rc_corr_lookup_chain_conv / rc_corr_lookup_chain_conv_backward (the fused
lookup + convc1 on the pair layout): what the C-ABI accepts
and what it refuses, all before any launch -- no GPU needed (B = 0 with fake
pointers, as in test_out_dtype_host.py) -- the unchanged ABI version, the
binding's message for a library without the symbols, and the Python keyword's
argument check."""
import ctypes
import os

import pytest
import torch

import raft_stereo_amd  # noqa: F401  (registered by conftest)
from raft_stereo_amd import CorrBlock1D, _lib

P = ctypes.c_void_p
TWO = (lambda: _lib.ptr_array([P(0x1000), None]), lambda: _lib.int_array([64, 32]), 2)
FOUR = (lambda: _lib.ptr_array([P(0x1000), None, P(0x2000), None]), lambda: _lib.int_array([64, 32, 16, 8]), 4)


def fwd(dt, ptrs, w, levels, B=0, radius=4, cout=8, weight=P(0x4000)):
    return _lib.lib().rc_corr_lookup_chain_conv(ptrs, w, None, dt, levels, radius, P(0x2000), 0, B, 1, 64,
                                                weight, P(0x5000), cout, 1, P(0x3000), None)


def bwd(dt, ptrs, w, levels, B=0, radius=4, cout=8, weight=P(0x4000), gc=P(0x6000)):
    return _lib.lib().rc_corr_lookup_chain_conv_backward(ptrs, w, None, dt, levels, radius, P(0x2000), 0, B, 1,
                                                         64, weight, P(0x5000), cout, 1, P(0x3000), gc, None,
                                                         None, None, None)


def test_abi_version_unchanged():
    assert _lib.lib().rc_abi_version() == _lib.ABI_VERSION == 13


@pytest.mark.parametrize("layout", [TWO, FOUR], ids=["2-levels", "4-levels"])
@pytest.mark.parametrize("elem", ["RC_F32", "RC_BF16"])
def test_forward_accepts(layout, elem):
    """Each pyramid dtype x output dtype x shadow choice passes every check
    of the forward for [p, NULL] and [p, NULL, p, NULL] (B = 0: RC_OK after
    the checks, nothing launched)."""
    ptrs, w, levels = layout
    for out in (0, _lib.RC_OUT_F16, _lib.RC_OUT_BF16):
        for sh in (0, _lib.RC_SHADOW, _lib.shadow_level(0)):
            dt = getattr(_lib, elem) | out | sh
            assert fwd(dt, ptrs(), w(), levels) == _lib.RC_OK, (elem, hex(out), hex(sh))
    # the backward takes the same layouts and shadow flags (its empty problem
    # would zero the sums through the runtime, so only its checks run here:
    # grad_corr alone requested)
    for sh in (0, _lib.RC_SHADOW, _lib.shadow_level(0)):
        assert bwd(getattr(_lib, elem) | sh, ptrs(), w(), levels) == _lib.RC_OK


@pytest.mark.parametrize("call", [fwd, bwd], ids=["forward", "backward"])
@pytest.mark.parametrize("B", [0, 1])
def test_refusals(call, B):
    """RC_EUNSUPPORTED with a message, before any launch and whatever B is."""
    L = _lib.lib()

    def refused(rc, code=_lib.RC_EUNSUPPORTED):
        assert rc == code
        assert L.rc_last_error()

    ptrs, w, levels = FOUR
    for flag in (_lib.RC_OUT_CHANNELS_LAST, _lib.RC_LAYOUT_RECORDS, _lib.RC_LAYOUT_DISPARITY):
        refused(call(_lib.RC_F32 | flag, ptrs(), w(), levels, B=B))
        refused(call(_lib.RC_BF16 | flag, ptrs(), w(), levels, B=B))
    refused(call(_lib.RC_BF16 | _lib.RC_LAYOUT_RECORDS, _lib.ptr_array([P(0x1000), None, None, None]),
                 _lib.int_array([128, 64, 32, 16]), 4, B=B))
    # 3 levels (the level-1 chain), with and without level 2
    w3 = _lib.int_array([64, 32, 16])
    refused(call(_lib.RC_F32, _lib.ptr_array([P(0x1000), P(0x2000), None]), w3, 3, B=B))
    refused(call(_lib.RC_F32, _lib.ptr_array([P(0x1000), None, P(0x2000)]), w3, 3, B=B))
    # 4 levels without level 2
    refused(call(_lib.RC_F32, _lib.ptr_array([P(0x1000), P(0x2000), None, None]), w(), 4, B=B))
    refused(call(_lib.RC_F32, _lib.ptr_array([P(0x1000), None, None, None]), w(), 4, B=B))
    refused(call(_lib.RC_F32, _lib.ptr_array([P(0x1000), P(0x2000), None, P(0x3000)]), w(), 4, B=B))
    # rc_corr_lookup_chain's own checks
    refused(call(_lib.RC_F32, ptrs(), w(), levels, B=B, radius=5))
    refused(call(_lib.RC_F32, ptrs(), _lib.int_array([1 << 17, 1 << 16, 1 << 15, 1 << 14]), levels, B=B))
    refused(call(_lib.RC_F32, ptrs(), _lib.int_array([64, 32, 16, 9]), levels, B=B), _lib.RC_EINVAL)
    refused(call(_lib.RC_F32 | 0x400000, ptrs(), w(), levels, B=B), _lib.RC_EINVAL)
    refused(call(7, ptrs(), w(), levels, B=B), _lib.RC_EINVAL)
    refused(call(_lib.RC_F32, ptrs(), w(), levels, B=B, cout=0), _lib.RC_EINVAL)


def test_out_flags():
    """Forward: either flag selects out's element type, both are RC_EINVAL.
    Backward: grad_out and the gradients are fp32, the flags RC_EUNSUPPORTED."""
    L = _lib.lib()
    ptrs, w, levels = FOUR
    both = _lib.RC_OUT_F16 | _lib.RC_OUT_BF16
    for B in (0, 1):
        assert fwd(_lib.RC_F32 | both, ptrs(), w(), levels, B=B) == _lib.RC_EINVAL and L.rc_last_error()
        for flag in (_lib.RC_OUT_F16, _lib.RC_OUT_BF16, both):
            assert bwd(_lib.RC_F32 | flag, ptrs(), w(), levels, B=B) == _lib.RC_EUNSUPPORTED
            assert L.rc_last_error()


def test_work_to_do_needs_its_pointers():
    """With pixels to process: a null weight, a null level 0, a misaligned
    level and a backward that asks for nothing are RC_EINVAL (checked before
    the launch; nothing runs here)."""
    L = _lib.lib()
    ptrs, w, levels = FOUR
    for call in (fwd, bwd):
        assert call(_lib.RC_F32, ptrs(), w(), levels, B=1, weight=None) == _lib.RC_EINVAL
        assert b"weight" in L.rc_last_error()
        assert call(_lib.RC_F32, _lib.ptr_array([None, None, P(0x2000), None]), w(), levels, B=1) == _lib.RC_EINVAL
        assert call(_lib.RC_F32, _lib.ptr_array([P(0x1004), None, P(0x2000), None]), w(), levels,
                    B=1) == _lib.RC_EINVAL
    assert bwd(_lib.RC_F32, ptrs(), w(), levels, B=1, gc=None) == _lib.RC_EINVAL
    # a row stride that is not whole 16-B chunks (the pair kernel's loads)
    w6 = _lib.int_array([66, 33])
    assert fwd(_lib.RC_F32, _lib.ptr_array([P(0x1000), None]), w6, 2, B=1) == _lib.RC_EINVAL
    assert b"stride" in L.rc_last_error()


def test_per_level_entry_points_keep_their_refusals():
    """rc_corr_lookup_conv still needs every level and still refuses the out flags."""
    L = _lib.lib()
    ptrs, w, levels = FOUR
    rc = L.rc_corr_lookup_conv(ptrs(), w(), None, _lib.RC_F32, levels, 4, P(0x2000), 0, 1, 1, 64, P(0x4000), None,
                               8, 1, P(0x3000), None)
    assert rc == _lib.RC_EINVAL and L.rc_last_error()
    rc = L.rc_corr_lookup_conv(ptrs(), w(), None, _lib.RC_F32 | _lib.RC_OUT_F16, levels, 4, P(0x2000), 0, 0, 1, 64,
                               P(0x4000), None, 8, 1, P(0x3000), None)
    assert rc == _lib.RC_EUNSUPPORTED and L.rc_last_error()


def test_stale_library_is_named(tmp_path, monkeypatch):
    """A library without one of the bound symbols (built before an entry
    point was added within the ABI version) raises CorrLibError asking for a
    rebuild, not a bare AttributeError."""
    monkeypatch.setitem(_lib.SIGNATURES, "rc_not_in_this_library", (ctypes.c_int, []))
    with pytest.raises(_lib.CorrLibError, match="rebuild the library"):
        _lib._open(_lib.LIB_PATH)
    assert os.path.exists(_lib.LIB_PATH)


def test_python_keyword_checks_its_argument():
    """out_dtype of lookup_convc1 is validated first: a bad value raises
    ValueError before any tensor is looked at."""
    blk = CorrBlock1D.__new__(CorrBlock1D)          # no build: the check comes first
    z = torch.zeros(1, 2, 1, 16)
    w = torch.zeros(8, 36)
    with pytest.raises(ValueError, match="out_dtype"):
        blk.lookup_convc1(z, w, out_dtype=torch.float64)
    with pytest.raises(ValueError, match="out_dtype"):
        blk.lookup_convc1(z, w, out_dtype="half")
    from raft_stereo_amd import corr
    with pytest.raises(ValueError, match="out_dtype"):
        corr.lookup_chain_convc1([torch.zeros(16, 1, 1, 16), None], z, 2, 4, w, out_dtype=torch.float64)
