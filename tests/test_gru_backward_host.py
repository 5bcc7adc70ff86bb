"""rc_gru_gates_backward / rc_gru_blend_backward and the training route of the
fused ConvGRU, as far as no GPU is needed: what the C-ABI
accepts and refuses before any launch (fake pointers; N = 0 wherever the
checks pass, N = 1 only where they refuse), the binding, the ``differentiable``
keyword of ``gru.why_not_fusable``, the ``fuse_gru_backward`` keyword's effect
on the module tree, and CPU modules, which keep running the PyTorch ops."""
import ctypes

import pytest
import torch

import raft_stereo_amd  # noqa: F401  (registered by conftest)
from raft_stereo_amd import _lib, gru
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


def gates(dtype=_lib.RC_F32, N=0, C=C, HW=HW, strides=None, triples=(PLANAR,) * 9, **kw):
    s = _lib.long_array([v for t in triples for v in t]) if strides is None else strides
    return _lib.lib().rc_gru_gates_backward(*ptrs(9, **kw), s, dtype, N, C, HW, None)


def blend(dtype=_lib.RC_F32, N=0, C=C, HW=HW, strides=None, triples=(PLANAR,) * 8, **kw):
    s = _lib.long_array([v for t in triples for v in t]) if strides is None else strides
    return _lib.lib().rc_gru_blend_backward(*ptrs(8, **kw), s, dtype, N, C, HW, None)


CALLS = [(gates, 9), (blend, 8)]
IDS = ["gates", "blend"]


def test_abi_version_unchanged_and_symbols_bound():
    assert _lib.lib().rc_abi_version() == _lib.ABI_VERSION == 13
    assert len(_lib.SIGNATURES["rc_gru_gates_backward"][1]) == 15
    assert len(_lib.SIGNATURES["rc_gru_blend_backward"][1]) == 14


@pytest.mark.parametrize("call,n", CALLS, ids=IDS)
def test_accepts(call, n):
    """Every dtype, both layout classes, slices of larger buffers, the strides
    of a length-1 axis ignored: RC_OK with nothing to do (N = 0, H*W = 0),
    null pointers included."""
    for dt in DTYPES:
        assert call(dt) == _lib.RC_OK
        assert call(dt, triples=(INTER,) * n) == _lib.RC_OK
        assert call(dt, N=3, HW=0) == _lib.RC_OK
    for k in range(n):
        assert call(N=0, null=k) == _lib.RC_OK
    # g_zpre / g_rpre as the halves of one stacked (N, 2C) buffer
    stacked = tuple((2 * C * HW, HW, 1) if k in (n - 3, n - 2) else PLANAR for k in range(n))
    assert call(triples=stacked) == _lib.RC_OK
    assert call(triples=((HW * 11, 1, 11),) + (INTER,) * (n - 1)) == _lib.RC_OK
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
    RC_EINVAL and named; 2^32 work units and more are RC_EUNSUPPORTED (all
    before the launch; nothing runs here)."""
    L = _lib.lib()
    for k in range(n):
        assert call(N=1, null=k) == _lib.RC_EINVAL
        assert b"null" in L.rc_last_error()
        assert call(_lib.RC_BF16, N=1, odd=k) == _lib.RC_EINVAL
        assert b"aligned" in L.rc_last_error()
    assert call(N=1 << 20, C=1 << 10, HW=4, triples=((4 << 10, 4, 1),) * n) == _lib.RC_EUNSUPPORTED


@pytest.mark.parametrize("name,n", [("rc_gru_gates_backward", 9), ("rc_gru_blend_backward", 8)], ids=IDS)
def test_two_outputs_must_not_alias(name, n):
    s = _lib.long_array(list(PLANAR) * n)
    fn = getattr(_lib.lib(), name)
    for i, k in ((n - 3, n - 2), (n - 3, n - 1), (n - 2, n - 1)):
        p = ptrs(n)
        p[k] = p[i]
        assert fn(*p, s, _lib.RC_F32, 1, C, HW, None) == _lib.RC_EINVAL
        assert b"alias" in _lib.lib().rc_last_error()
        assert fn(*p, s, _lib.RC_F32, 0, C, HW, None) == _lib.RC_OK


def test_wrappers_have_no_cpu_fallback():
    t = torch.zeros(1, 4, 3, 5)
    with pytest.raises(RuntimeError, match="HIP"):
        gru.gru_gates_backward(t, t, t, t, t, t)
    with pytest.raises(RuntimeError, match="HIP"):
        gru.gru_blend_backward(t, t, t, t, t)


def cpu_case():
    torch.manual_seed(0)
    m = ConvGRU(8, 12).eval()
    g = torch.Generator().manual_seed(1)
    return m, [torch.randn(1, 8, 5, 6, generator=g) for _ in range(4)] + [torch.randn(1, 12, 5, 6, generator=g)]


def test_differentiable_skips_only_the_gradient_reason():
    m, args = cpu_case()
    args[0].requires_grad_(True)
    assert "gradient" in gru.why_not_fusable(m, *args)
    why = gru.why_not_fusable(m, *args, differentiable=True)
    assert "HIP devices only" in why and "gradient" not in why
    assert not gru.fusable(m, *args, differentiable=True)
    # every other condition still holds
    assert "mixed dtypes" in gru.why_not_fusable(m, args[0], args[1].bfloat16(), *args[2:], differentiable=True)
    assert "float64" in gru.why_not_fusable(m, *[t.double() for t in args], differentiable=True)
    assert gru.why_not_fusable(m, *args[:4], differentiable=True) is not None          # no x at all
    for p in m.parameters():
        p.requires_grad_(False)
    h = args[0].detach()
    assert "HIP devices only" in gru.why_not_fusable(m, h, *args[1:])
    assert "HIP devices only" in gru.why_not_fusable(m, h, *args[1:], differentiable=True)


def test_fuse_gru_backward_keyword():
    with pytest.raises(ValueError, match="fuse_gru"):
        RAFTStereo(StereoArgs(), fuse_gru_backward=True)
    torch.manual_seed(0)
    base = RAFTStereo(StereoArgs())
    torch.manual_seed(0)
    train = RAFTStereo(StereoArgs(), fuse_gru=True, fuse_gru_backward=True)
    assert list(train.state_dict()) == list(base.state_dict())
    assert all(torch.equal(a, b) for a, b in zip(train.state_dict().values(), base.state_dict().values()))
    ub = train.update_block
    assert train.fuse_gru and train.fuse_gru_backward
    assert all(getattr(ub, n).fuse and getattr(ub, n).fuse_backward for n in ("gru08", "gru16", "gru32"))
    ub = RAFTStereo(StereoArgs(), fuse_gru=True).update_block
    assert all(getattr(ub, n).fuse and not getattr(ub, n).fuse_backward for n in ("gru08", "gru16", "gru32"))
    assert not base.fuse_gru_backward and ConvGRU(8, 8).fuse_backward is False


def test_cpu_module_runs_the_torch_ops_forward_and_backward():
    """``fuse`` and ``fuse_backward`` set, CPU tensors: not fusable, so the
    output and every gradient are the unfused module's bit for bit."""
    outs = []
    for fuse in (False, True):
        m, args = cpu_case()
        m.fuse = m.fuse_backward = fuse
        for t in args:
            t.requires_grad_(True)
        out = m(*args)
        torch.manual_seed(2)
        out.backward(torch.randn(out.shape))
        outs.append([out.detach()] + [t.grad for t in args] + [p.grad for p in m.parameters()])
    assert len(outs[0]) == 1 + 5 + 6 and all(t is not None for t in outs[1])
    assert all(torch.equal(a, b) for a, b in zip(*outs))
