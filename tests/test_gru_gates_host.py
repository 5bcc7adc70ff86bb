"""rc_gru_gates / rc_gru_blend (the ConvGRU glue kernels): what
the C-ABI accepts and what it refuses, all before any launch -- no GPU needed
(fake pointers; N = 0 wherever the checks pass, N = 1 only where they refuse)
-- the unchanged ABI version, the binding, ``gru.fusable``'s refusals on CPU
tensors and the ``fuse_gru`` keyword's effect on the module tree."""
import ctypes

import pytest
import torch

import raft_stereo_amd  # noqa: F401  (registered by conftest)
from raft_stereo_amd import _lib, gru, shard
from raft_stereo_amd.network import ConvGRU, RAFTStereo, StereoArgs

P = ctypes.c_void_p
C, HW = 8, 15
PLANAR = (C * HW, HW, 1)
INTER = (HW * C, 1, C)
DTYPES = [_lib.RC_F32, _lib.RC_F16, _lib.RC_BF16]


def ptrs(n, null=None, odd=None):
    out = [P(0x1000 * (k + 1)) for k in range(n)]
    if null is not None:
        out[null] = None
    if odd is not None:
        out[odd] = P(0x1000 * (odd + 1) + 1)
    return out


def gates(dtype=_lib.RC_F32, N=0, C=C, HW=HW, strides=None, triples=(PLANAR,) * 7, **kw):
    s = _lib.long_array([v for t in triples for v in t]) if strides is None else strides
    return _lib.lib().rc_gru_gates(*ptrs(7, **kw), s, dtype, N, C, HW, None)


def blend(dtype=_lib.RC_F32, N=0, C=C, HW=HW, strides=None, triples=(PLANAR,) * 5, **kw):
    s = _lib.long_array([v for t in triples for v in t]) if strides is None else strides
    return _lib.lib().rc_gru_blend(*ptrs(5, **kw), s, dtype, N, C, HW, None)


CALLS = [(gates, 7), (blend, 5)]
IDS = ["gates", "blend"]


def test_abi_version_unchanged_and_symbols_bound():
    assert _lib.lib().rc_abi_version() == _lib.ABI_VERSION == 13
    assert "rc_gru_gates" in _lib.SIGNATURES and "rc_gru_blend" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["rc_gru_gates"][1]) == 13 and len(_lib.SIGNATURES["rc_gru_blend"][1]) == 11


@pytest.mark.parametrize("call,n", CALLS, ids=IDS)
def test_accepts(call, n):
    """Every dtype, both layout classes, slices of larger buffers (other batch
    and row strides), the strides of a length-1 axis ignored: RC_OK with
    nothing to do (N = 0, H*W = 0)."""
    for dt in DTYPES:
        assert call(dt) == _lib.RC_OK
        assert call(dt, triples=(INTER,) * n) == _lib.RC_OK
        assert call(dt, N=3, HW=0) == _lib.RC_OK
    sliced = ((3 * C * HW, HW, 1),) * 2 + (PLANAR,) * (n - 2)
    assert call(triples=sliced) == _lib.RC_OK
    sliced = ((HW * 11, 1, 11),) + (INTER,) * (n - 1)
    assert call(triples=sliced) == _lib.RC_OK
    # C == 1: the channel stride says nothing; H*W == 1: the pixel stride
    assert call(C=1, triples=((HW, 77, 1),) + ((HW, 1, 1),) * (n - 1)) == _lib.RC_OK
    assert call(HW=1, triples=((C, 1, 5),) + ((C, 1, 1),) * (n - 1)) == _lib.RC_OK


@pytest.mark.parametrize("N", [0, 1])
@pytest.mark.parametrize("call,n", CALLS, ids=IDS)
def test_refusals(call, n, N):
    """With a message, before any launch and whatever N is."""
    L = _lib.lib()

    def refused(rc, code, word=None):
        assert rc == code
        assert L.rc_last_error()
        assert word is None or word in L.rc_last_error()

    for dt in (3, 7, -1, _lib.RC_F32 | 0x100):
        refused(call(dt, N=N), _lib.RC_EINVAL, b"dtype")
    refused(call(N=N, C=0), _lib.RC_EINVAL)
    refused(call(N=N, C=-4), _lib.RC_EINVAL)
    refused(call(N=-1), _lib.RC_EINVAL)
    refused(call(N=N, HW=-1), _lib.RC_EINVAL)
    refused(call(N=N, strides=ctypes.POINTER(ctypes.c_long)()), _lib.RC_EINVAL, b"stride")
    refused(call(N=N, triples=((C * HW, -HW, 1),) + (PLANAR,) * (n - 1)), _lib.RC_EINVAL, b"stride")
    # mixed layout classes: one interleaved operand among planar ones, each
    # position; and an operand of neither class
    for k in range(n):
        mixed = tuple(INTER if i == k else PLANAR for i in range(n))
        refused(call(N=N, triples=mixed), _lib.RC_EUNSUPPORTED, b"layout")
    refused(call(N=N, triples=((2 * C * HW, 2 * HW, 2),) * n), _lib.RC_EUNSUPPORTED, b"layout")


@pytest.mark.parametrize("call,n", CALLS, ids=IDS)
def test_work_to_do_needs_its_operands(call, n):
    """N*H*W > 0: a null operand and one not aligned to its element size are
    RC_EINVAL and named (checked before the launch; nothing runs here)."""
    L = _lib.lib()
    for k in range(n):
        assert call(N=1, null=k) == _lib.RC_EINVAL
        assert b"null" in L.rc_last_error()
        assert call(N=0, null=k) == _lib.RC_OK
        assert call(_lib.RC_BF16, N=1, odd=k) == _lib.RC_EINVAL
        assert b"aligned" in L.rc_last_error()
    # 2^32 elements and more
    assert call(N=1 << 20, C=1 << 10, HW=4, triples=((4 << 10, 4, 1),) * n) == _lib.RC_EUNSUPPORTED


def test_rh_out_must_not_be_h():
    s = _lib.long_array(list(PLANAR) * 7)
    p = ptrs(7)
    p[6] = p[4]
    assert _lib.lib().rc_gru_gates(*p, s, _lib.RC_F32, 1, C, HW, None) == _lib.RC_EINVAL
    assert b"alias" in _lib.lib().rc_last_error()


def test_wrappers_have_no_cpu_fallback():
    t = torch.zeros(1, 4, 3, 5)
    with pytest.raises(RuntimeError, match="HIP"):
        gru.gru_gates(t, t, t, t, t)
    with pytest.raises(RuntimeError, match="HIP"):
        gru.gru_blend(t, t, t, t)


def test_fusable_refusals_on_cpu_tensors():
    torch.manual_seed(0)
    m = ConvGRU(8, 12).eval()
    h, cz, cr, cq = (torch.randn(1, 8, 5, 6) for _ in range(4))
    x = torch.randn(1, 12, 5, 6)
    with torch.no_grad():
        assert not gru.fusable(m, h, cz, cr, cq, x)
        assert "HIP devices only" in gru.why_not_fusable(m, h, cz, cr, cq, x)
        assert not gru.fusable(m, h, cz.bfloat16(), cr, cq, x)
        assert "mixed dtypes" in gru.why_not_fusable(m, h, cz.bfloat16(), cr, cq, x)
        assert not gru.fusable(m, h, cz, cr, cq, x.half())
        assert "mixed dtypes" in gru.why_not_fusable(m, h, cz, cr, cq, x.half())
        d = [t.double() for t in (h, cz, cr, cq, x)]
        assert not gru.fusable(m, *d)
        assert "float64" in gru.why_not_fusable(m, *d)
        assert not gru.fusable(m, h, cz, cr, cq)                       # no x at all
        assert not gru.fusable(m, h, cz, cr, cq[:, :, :4], x)
    for p in m.parameters():
        p.requires_grad_(False)
    assert "HIP devices only" in gru.why_not_fusable(m, h, cz, cr, cq, x)    # grad mode, nothing to record
    hg = h.clone().requires_grad_(True)
    assert not gru.fusable(m, hg, cz, cr, cq, x)
    assert "gradient" in gru.why_not_fusable(m, hg, cz, cr, cq, x)
    with torch.no_grad():
        assert "HIP devices only" in gru.why_not_fusable(m, hg, cz, cr, cq, x)
    m.convq.weight.requires_grad_(True)
    assert "gradient" in gru.why_not_fusable(m, h, cz, cr, cq, x)


def test_layout_classes_and_pixel_merge():
    t = torch.zeros(2, 6, 4, 5)
    assert gru._classes(t) == {"planar"} and gru._triple(t) == (120, 20, 1)
    cl = t.contiguous(memory_format=torch.channels_last)
    assert gru._classes(cl) == {"interleaved"} and gru._triple(cl) == (120, 1, 6)
    assert gru._classes(cl[:, :4]) == {"interleaved"} and gru._triple(cl[:, 2:4]) == (120, 1, 6)
    assert gru._triple(t[:, :, :, :3]) is None and not gru._classes(t[:, :, :, :3])     # rows do not merge
    assert gru._triple(t[:, :, :2]) == (120, 20, 1)
    assert gru._classes(t[:, :1]) == {"planar", "interleaved"}
    assert not gru._common_class((t, cl))


def test_fuse_gru_keeps_the_module_tree():
    torch.manual_seed(0)
    base = RAFTStereo(StereoArgs())
    torch.manual_seed(0)
    fused = RAFTStereo(StereoArgs(), fuse_gru=True)
    assert list(fused.state_dict()) == list(base.state_dict())
    assert all(torch.equal(a, b) for a, b in zip(fused.state_dict().values(), base.state_dict().values()))
    ub = fused.update_block
    assert fused.fuse_gru and ub.gru08.fuse and ub.gru16.fuse and ub.gru32.fuse
    ub = base.update_block
    assert not (base.fuse_gru or ub.gru08.fuse or ub.gru16.fuse or ub.gru32.fuse)
    assert ConvGRU(8, 8).fuse is False


def test_fused_module_on_cpu_runs_the_torch_ops():
    """``fuse`` set, CPU tensors: not fusable, so forward is the unfused code."""
    torch.manual_seed(0)
    m = ConvGRU(8, 12).eval()
    args = [torch.randn(1, 8, 5, 6) for _ in range(4)] + [torch.randn(1, 12, 5, 6)]
    with torch.no_grad():
        want = m(*args)
        m.fuse = True
        assert torch.equal(m(*args), want)


def test_stacked_conv_keeps_its_old_names():
    assert shard._zr_conv is gru._zr_conv and shard._ZR is gru._ZR
    torch.manual_seed(0)
    m = ConvGRU(8, 12).eval()
    with torch.no_grad():
        w, b, c = gru._zr_conv_as(m, torch.bfloat16)
        w2, _, _ = gru._zr_conv_as(m, torch.bfloat16)
        assert w.dtype == b.dtype == torch.bfloat16 and c == 8 and w2 is w
        m.convr.weight.mul_(2.0)
        w3, _, _ = gru._zr_conv_as(m, torch.bfloat16)
        assert torch.equal(w3[8:], m.convr.weight.bfloat16()) and not torch.equal(w3[8:], w[8:])
        assert gru._zr_conv_as(m, torch.float32)[0] is gru._zr_conv(m)[0]
