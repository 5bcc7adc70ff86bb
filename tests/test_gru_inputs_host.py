"""rc_gru_assemble (the ConvGRU input assembly): what the C ABI
accepts and what it refuses, all before any launch -- no GPU needed (fake
pointers; wherever the checks pass there is nothing to do: N, H or W is 0) --
the unchanged ABI version, the binding, the ``Pooled`` / ``Resized``
descriptors on CPU tensors and the ``fuse_gru_inputs`` keyword."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import raft_stereo_amd  # noqa: F401  (registered by conftest)
from oracle import torch_ref
from raft_stereo_amd import _lib, gru, network
from raft_stereo_amd.network import ConvGRU, RAFTStereo, StereoArgs

COPY, POOL, BIL = _lib.RC_PART_COPY, _lib.RC_PART_POOL2X, _lib.RC_PART_BILINEAR
H, W = 3, 5
# (mode, channels, src_h, src_w): h, a pooled part and a resized one
PARTS = [(COPY, 8, H, W), (POOL, 3, 5, 9), (BIL, 5, 2, 3)]


def planar(C, h, w):
    return (C * h * w, h * w, w, 1)


def inter(C, h, w):
    return (h * w * C, 1, w * C, C)


def call(N=1, H=H, W=W, parts=PARTS, dst=0x10000, dst_strides=None, dst_dtype=_lib.RC_F32, nparts=None,
         src=None, src_strides=None, src_dtype=None, mode=None, channels=None, src_h=None, src_w=None,
         drop=()):
    """rc_gru_assemble on fake pointers.  Every array argument is built from
    ``parts`` unless given; ``drop`` names the arguments passed as NULL."""
    C = sum(p[1] for p in parts)
    n = len(parts)
    args = {
        "dst": ctypes.c_void_p(dst),
        "dst_strides": _lib.long_array(planar(C, H, W) if dst_strides is None else dst_strides),
        "src": _lib.ptr_array([0x100000 * (i + 1) for i in range(n)] if src is None else src),
        "src_strides": _lib.long_array([v for p in parts for v in planar(p[1], p[2], p[3])]
                                       if src_strides is None else src_strides),
        "src_dtype": _lib.int_array([_lib.RC_F32] * n if src_dtype is None else src_dtype),
        "mode": _lib.int_array([p[0] for p in parts] if mode is None else mode),
        "channels": _lib.int_array([p[1] for p in parts] if channels is None else channels),
        "src_h": _lib.int_array([p[2] for p in parts] if src_h is None else src_h),
        "src_w": _lib.int_array([p[3] for p in parts] if src_w is None else src_w),
    }
    for name in drop:
        args[name] = None
    return _lib.lib().rc_gru_assemble(
        args["dst"], args["dst_strides"], dst_dtype, N, H, W, n if nparts is None else nparts, args["src"],
        args["src_strides"], args["src_dtype"], args["mode"], args["channels"], args["src_h"], args["src_w"],
        None)


def refused(rc, code, word):
    err = _lib.lib().rc_last_error()
    assert rc == code, (rc, err)
    assert word in err, err


def test_abi_version_unchanged_and_symbol_bound():
    assert _lib.lib().rc_abi_version() == _lib.ABI_VERSION == 13
    assert "rc_gru_assemble" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["rc_gru_assemble"][1]) == 15
    assert (_lib.RC_GRU_MAX_PARTS, COPY, POOL, BIL) == (4, 0, 1, 2)
    assert hasattr(_lib.lib(), "rc_gru_assemble")


def test_empty_is_ok():
    """N, H or W equal to 0: RC_OK, nothing launched (the pointers are fake)."""
    assert call(N=0) == _lib.RC_OK
    assert call(N=2, H=0, parts=[(BIL, 4, 2, 3)]) == _lib.RC_OK
    assert call(N=2, W=0, parts=[(BIL, 4, 2, 3)]) == _lib.RC_OK
    for dt in (_lib.RC_F32, _lib.RC_F16, _lib.RC_BF16):
        assert call(N=0, dst_dtype=dt, src_dtype=[dt, _lib.RC_F32, _lib.RC_BF16]) == _lib.RC_OK
    C = sum(p[1] for p in PARTS)
    assert call(N=0, dst_strides=inter(C, H, W)) == _lib.RC_OK
    # a channel slice of a wider buffer, planar and interleaved
    assert call(N=0, dst_strides=planar(C + 7, H, W)) == _lib.RC_OK
    assert call(N=0, dst_strides=inter(C + 7, H, W)) == _lib.RC_OK
    # crossed: interleaved sources of a planar dst
    assert call(N=0, src_strides=[v for p in PARTS for v in inter(p[1], p[2], p[3])]) == _lib.RC_OK
    assert call(N=0, parts=[(COPY, 1, H, W)] * 4) == _lib.RC_OK


@pytest.mark.parametrize("N", [0, 1])
def test_einval_names_the_argument(N):
    """With a message that names the argument, before any launch, whatever N is."""
    E = _lib.RC_EINVAL
    refused(call(N=N, nparts=0), E, b"nparts")
    refused(call(N=N, nparts=5), E, b"nparts")
    refused(call(N=N, nparts=-1), E, b"nparts")
    for name in ("dst_strides", "src", "src_strides", "src_dtype", "mode", "channels", "src_h", "src_w"):
        refused(call(N=N, drop=(name,)), E, name.encode())
    refused(call(N=N, dst=None), E, b"dst")
    refused(call(N=N, src=[0x100000, None, 0x300000]), E, b"src[1]")
    for dt in (3, 7, -1, 0x100):
        refused(call(N=N, dst_dtype=dt), E, b"dst_dtype")
        refused(call(N=N, src_dtype=[_lib.RC_F32, _lib.RC_F32, dt]), E, b"src_dtype[2]")
    for m in (3, -1, 16):
        refused(call(N=N, mode=[COPY, m, BIL]), E, b"mode[1]")
    refused(call(N=N, channels=[8, 0, 5]), E, b"channels[1]")
    refused(call(N=N, channels=[8, 3, -2]), E, b"channels[2]")
    # COPY of another size
    refused(call(N=N, src_h=[H + 1, 5, 2]), E, b"RC_PART_COPY")
    refused(call(N=N, src_w=[W - 1, 9, 3]), E, b"RC_PART_COPY")
    # POOL2X whose source does not pool to H x W: 7 rows give 4, 11 columns give 6
    refused(call(N=N, src_h=[H, 7, 2]), E, b"RC_PART_POOL2X")
    refused(call(N=N, src_w=[W, 11, 3]), E, b"RC_PART_POOL2X")
    refused(call(N=N, src_w=[W, 8, 3]), E, b"RC_PART_POOL2X")        # 8 columns give 4
    # BILINEAR from nothing
    refused(call(N=N, src_h=[H, 5, 0]), E, b"src_h[2]")
    refused(call(N=N, src_w=[W, 9, -1]), E, b"src_w[2]")
    # dst is a source
    refused(call(N=N, src=[0x100000, 0x10000, 0x300000]), E, b"dst")
    # negative sizes and strides
    refused(call(N=-1), E, b"N=")
    refused(call(N=N, dst_strides=(120, -15, 5, 1)), E, b"dst_strides")
    neg = [v for p in PARTS for v in planar(p[1], p[2], p[3])]
    neg[5] = -1
    refused(call(N=N, src_strides=neg), E, b"src_strides")


def test_pool_accepts_even_and_odd_sources():
    assert call(N=0, parts=[(POOL, 2, 5, 9), (POOL, 2, 6, 10)]) == _lib.RC_OK
    assert call(N=0, H=1, W=8, parts=[(POOL, 4, 1, 15), (POOL, 4, 2, 16), (BIL, 4, 1, 1)]) == _lib.RC_OK


@pytest.mark.parametrize("N", [0, 1])
def test_unsupported_dst_layouts(N):
    """Neither planar nor interleaved: RC_EUNSUPPORTED before any launch."""
    U = _lib.RC_EUNSUPPORTED
    C = sum(p[1] for p in PARTS)
    refused(call(N=N, dst_strides=(2 * C * H * W, 2 * H * W, 2 * W, 2)), U, b"dst_strides")       # column stride 2
    refused(call(N=N, dst_strides=(C * H * (W + 3), H * (W + 3), W + 3, 1)), U, b"dst_strides")    # padded rows
    refused(call(N=N, dst_strides=(H * W * C * 2, 2, W * C * 2, C * 2)), U, b"dst_strides")        # channel stride 2


def test_work_to_do_needs_aligned_pointers_and_a_size_under_2_31():
    refused(call(dst=0x10001, dst_dtype=_lib.RC_BF16), _lib.RC_EINVAL, b"aligned")
    refused(call(src=[0x100000, 0x200002, 0x300000]), _lib.RC_EINVAL, b"src[1]")
    big = [(COPY, 1 << 10, 1 << 10, 1 << 10)]
    refused(call(N=4, H=1 << 10, W=1 << 10, parts=big), _lib.RC_EUNSUPPORTED, b"2^31")


def test_descriptors_on_cpu_tensors():
    g = torch.Generator().manual_seed(0)
    for shape in [(2, 6, 17, 39), (1, 3, 10, 26), (1, 2, 1, 15), (1, 2, 7, 1)]:
        t = torch.randn(shape, generator=g)
        p = gru.Pooled(t)
        want = network.pool2x(t)
        assert p.shape == want.shape and p.dtype == t.dtype and p.device == t.device and p.dim() == 4
        assert not p.requires_grad
        assert torch.equal(p.materialize(), want)
        assert torch.equal(want, F.avg_pool2d(t, 3, stride=2, padding=1))
    t = torch.randn(2, 6, 5, 10, generator=g)
    dest = torch.empty(2, 1, 9, 20)
    r = gru.Resized(t, dest.shape[2:])
    want = network.interp(t, dest)
    assert r.shape == want.shape == (2, 6, 9, 20) and r.dtype == t.dtype and r.dim() == 4
    assert torch.equal(r.materialize(), want)
    assert gru.Pooled(t.requires_grad_(True)).requires_grad
    assert gru.materialized((t, gru.Pooled(t)))[0] is t
    with pytest.raises(TypeError):
        gru.Pooled("x")


def test_assemble_has_no_cpu_fallback():
    t = torch.zeros(1, 4, 3, 5)
    with pytest.raises(RuntimeError, match="HIP"):
        gru.assemble([t, gru.Pooled(torch.zeros(1, 2, 5, 9))], torch.float32, torch.contiguous_format)
    with torch.no_grad():
        assert "HIP devices only" in gru.why_not_assemblable([t], torch.float32, torch.contiguous_format)
        assert "parts" in gru.why_not_assemblable([], torch.float32, torch.contiguous_format)
        assert "parts" in gru.why_not_assemblable([t] * 5, torch.float32, torch.contiguous_format)
        assert "float64" in gru.why_not_assemblable([t], torch.float64, torch.contiguous_format)
        assert "differ" in gru.why_not_assemblable([t, gru.Pooled(torch.zeros(1, 2, 7, 9))], torch.float32)
    tg = t.clone().requires_grad_(True)
    assert "gradient" in gru.why_not_assemblable([tg], torch.float32, torch.contiguous_format)


def test_fusable_takes_descriptors():
    """``why_not_fusable`` sees a descriptor as its result: on CPU tensors the
    first reason is the device, not the part; a wrong size is named."""
    torch.manual_seed(0)
    m = ConvGRU(8, 12).eval()
    h, cz, cr, cq = (torch.randn(1, 8, 5, 6) for _ in range(4))
    with torch.no_grad():
        ok = (gru.Pooled(torch.randn(1, 6, 9, 11)), gru.Resized(torch.randn(1, 6, 3, 3), (5, 6)))
        assert "HIP devices only" in gru.why_not_fusable(m, h, cz, cr, cq, *ok)
        assert "shapes" in gru.why_not_fusable(m, h, cz, cr, cq, gru.Pooled(torch.randn(1, 12, 7, 11)))
        want = m(h, cz, cr, cq, *gru.materialized(ok))
        m.fuse = m.fuse_inputs = True
        assert torch.equal(m(h, cz, cr, cq, *ok), want)             # the unfused body materialises first
        m.fuse = False
        assert torch.equal(m(h, cz, cr, cq, *ok), want)


def test_keyword_needs_fuse_gru_and_keeps_the_module_tree():
    with pytest.raises(ValueError, match="fuse_gru"):
        RAFTStereo(StereoArgs(), fuse_gru_inputs=True)
    torch.manual_seed(0)
    base = RAFTStereo(StereoArgs())
    torch.manual_seed(0)
    fused = RAFTStereo(StereoArgs(), fuse_gru=True, fuse_gru_inputs=True)
    assert list(fused.state_dict()) == list(base.state_dict())
    ub = fused.update_block
    assert fused.fuse_gru_inputs and ub.fuse_inputs and ub.gru08.fuse_inputs and ub.gru16.fuse_inputs \
        and ub.gru32.fuse_inputs
    ub = base.update_block
    assert not (base.fuse_gru_inputs or ub.fuse_inputs or ub.gru08.fuse_inputs or ub.gru16.fuse_inputs
                or ub.gru32.fuse_inputs)
    assert ConvGRU(8, 8).fuse_inputs is False


def test_cpu_network_is_the_default_one_bit_for_bit():
    """On the CPU nothing is fusable: with both flags the descriptors are
    materialised by the torch ops and the predictions are the default
    network's."""
    g = torch.Generator().manual_seed(8)
    img1 = torch.rand(1, 3, 64, 96, generator=g) * 255
    img2 = torch.roll(img1, -4, dims=-1)
    outs = []
    for kw in ({}, {"fuse_gru": True, "fuse_gru_inputs": True}):
        torch.manual_seed(0)
        model = RAFTStereo(StereoArgs(), corr_block=torch_ref.TorchCorrBlock1D, **kw).eval()
        with torch.no_grad():
            outs.append(model(img1, img2, iters=2))
    assert len(outs[0]) == len(outs[1]) == 2
    assert all(torch.equal(a, b) for a, b in zip(*outs))

