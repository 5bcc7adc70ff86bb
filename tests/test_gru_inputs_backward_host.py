"""rc_gru_assemble_backward (the adjoint of the ConvGRU input assembly,
DESIGN.md §3.7): what the C ABI accepts and what it refuses, all before any
launch -- no GPU needed (fake pointers; wherever the checks pass there is
nothing to do: N, H or W is 0) -- the unchanged ABI version, the binding, the
``fuse_gru_inputs_backward`` keyword, and that with the option off or on CPU
tensors the PyTorch ops run, bit for bit."""
import ctypes

import pytest
import torch

import raft_stereo_amd  # noqa: F401  (registered by conftest)
from oracle import torch_ref
from raft_stereo_amd import _lib, gru
from raft_stereo_amd.network import ConvGRU, RAFTStereo, StereoArgs

COPY, POOL, BIL = _lib.RC_PART_COPY, _lib.RC_PART_POOL2X, _lib.RC_PART_BILINEAR
H, W = 3, 5
PARTS = [(COPY, 8, H, W), (POOL, 3, 5, 9), (BIL, 5, 2, 3)]
ALL = {"fuse_gru": True, "fuse_gru_backward": True, "fuse_gru_inputs": True, "fuse_gru_inputs_backward": True}


def planar(C, h, w):
    return (C * h * w, h * w, w, 1)


def inter(C, h, w):
    return (h * w * C, 1, w * C, C)


def call(N=1, H=H, W=W, parts=PARTS, g=0x10000, g2=None, g2_c0=0, g_strides=None, g_dtype=_lib.RC_F32, nparts=None,
         grad_src=None, grad_strides=None, grad_dtype=None, mode=None, channels=None, src_h=None, src_w=None,
         drop=()):
    """rc_gru_assemble_backward on fake pointers.  Every array argument is
    built from ``parts`` unless given; ``drop`` names the arguments passed as
    NULL."""
    C = sum(p[1] for p in parts)
    n = len(parts)
    args = {
        "g": ctypes.c_void_p(g),
        "g_strides": _lib.long_array(planar(C, H, W) if g_strides is None else g_strides),
        "grad_src": _lib.ptr_array([0x100000 * (i + 1) for i in range(n)] if grad_src is None else grad_src),
        "grad_strides": _lib.long_array([v for p in parts for v in planar(p[1], p[2], p[3])]
                                        if grad_strides is None else grad_strides),
        "grad_dtype": _lib.int_array([_lib.RC_F32] * n if grad_dtype is None else grad_dtype),
        "mode": _lib.int_array([p[0] for p in parts] if mode is None else mode),
        "channels": _lib.int_array([p[1] for p in parts] if channels is None else channels),
        "src_h": _lib.int_array([p[2] for p in parts] if src_h is None else src_h),
        "src_w": _lib.int_array([p[3] for p in parts] if src_w is None else src_w),
    }
    for name in drop:
        args[name] = None
    return _lib.lib().rc_gru_assemble_backward(
        args["g"], g2, g2_c0, args["g_strides"], g_dtype, N, H, W, n if nparts is None else nparts,
        args["grad_src"], args["grad_strides"], args["grad_dtype"], args["mode"], args["channels"], args["src_h"],
        args["src_w"], None)


def refused(rc, code, word):
    err = _lib.lib().rc_last_error()
    assert rc == code, (rc, err)
    assert word in err, err


def test_abi_version_unchanged_and_symbol_bound():
    assert _lib.lib().rc_abi_version() == _lib.ABI_VERSION == 13
    assert len(_lib.SIGNATURES["rc_gru_assemble_backward"][1]) == 17
    assert hasattr(_lib.lib(), "rc_gru_assemble_backward")


def test_empty_is_ok():
    """N, H or W equal to 0: RC_OK, nothing launched (the pointers are fake)."""
    assert call(N=0) == _lib.RC_OK
    assert call(N=2, H=0, parts=[(BIL, 4, 2, 3)]) == _lib.RC_OK
    assert call(N=2, W=0, parts=[(BIL, 4, 2, 3)]) == _lib.RC_OK
    for dt in (_lib.RC_F32, _lib.RC_F16, _lib.RC_BF16):
        assert call(N=0, g_dtype=dt, grad_dtype=[dt, _lib.RC_F32, _lib.RC_BF16]) == _lib.RC_OK
    C = sum(p[1] for p in PARTS)
    assert call(N=0, g_strides=inter(C, H, W)) == _lib.RC_OK
    assert call(N=0, g_strides=planar(C + 7, H, W)) == _lib.RC_OK
    assert call(N=0, g_strides=inter(C + 7, H, W)) == _lib.RC_OK
    assert call(N=0, grad_strides=[v for p in PARTS for v in inter(p[1], p[2], p[3])]) == _lib.RC_OK
    assert call(N=0, parts=[(COPY, 1, H, W)] * 4) == _lib.RC_OK
    # g2 and both ends of g2_c0; skipped parts, all but one
    assert call(N=0, g2=0x20000, g2_c0=0) == _lib.RC_OK
    assert call(N=0, g2=0x20000, g2_c0=8) == _lib.RC_OK
    assert call(N=0, g2=0x20000, g2_c0=C) == _lib.RC_OK
    assert call(N=0, grad_src=[None, 0x200000, 0x300000]) == _lib.RC_OK
    assert call(N=0, grad_src=[None, None, 0x300000]) == _lib.RC_OK
    # a downscale, 1-pixel sources and destinations
    assert call(N=0, H=3, W=4, parts=[(BIL, 4, 7, 9)]) == _lib.RC_OK
    assert call(N=0, H=1, W=8, parts=[(POOL, 4, 1, 15), (POOL, 4, 2, 16), (BIL, 4, 1, 1)]) == _lib.RC_OK


@pytest.mark.parametrize("N", [0, 1])
def test_einval_names_the_argument(N):
    """With a message that names the argument, before any launch, whatever N is."""
    E = _lib.RC_EINVAL
    C = sum(p[1] for p in PARTS)
    refused(call(N=N, nparts=0), E, b"nparts")
    refused(call(N=N, nparts=5), E, b"nparts")
    refused(call(N=N, nparts=-1), E, b"nparts")
    for name in ("g_strides", "grad_src", "grad_strides", "grad_dtype", "mode", "channels", "src_h", "src_w"):
        refused(call(N=N, drop=(name,)), E, name.encode())
    refused(call(N=N, g=None), E, b"null g")
    for dt in (3, 7, -1, 0x100):
        refused(call(N=N, g_dtype=dt), E, b"g_dtype")
        refused(call(N=N, grad_dtype=[_lib.RC_F32, _lib.RC_F32, dt]), E, b"grad_dtype[2]")
    for m in (3, -1, 16):
        refused(call(N=N, mode=[COPY, m, BIL]), E, b"mode[1]")
    refused(call(N=N, channels=[8, 0, 5]), E, b"channels[1]")
    refused(call(N=N, channels=[8, 3, -2]), E, b"channels[2]")
    refused(call(N=N, src_h=[H + 1, 5, 2]), E, b"RC_PART_COPY")
    refused(call(N=N, src_w=[W - 1, 9, 3]), E, b"RC_PART_COPY")
    refused(call(N=N, src_h=[H, 7, 2]), E, b"RC_PART_POOL2X")
    refused(call(N=N, src_w=[W, 11, 3]), E, b"RC_PART_POOL2X")
    refused(call(N=N, src_w=[W, 8, 3]), E, b"RC_PART_POOL2X")
    refused(call(N=N, src_h=[H, 5, 0]), E, b"src_h[2]")
    refused(call(N=N, src_w=[W, 9, -1]), E, b"src_w[2]")
    refused(call(N=-1), E, b"N=")
    refused(call(N=N, g_strides=(120, -15, 5, 1)), E, b"g_strides")
    neg = [v for p in PARTS for v in planar(p[1], p[2], p[3])]
    neg[5] = -1
    refused(call(N=N, grad_strides=neg), E, b"grad_strides")
    # what the adjoint adds: g2_c0, overlapping outputs, nothing to compute
    refused(call(N=N, g2=0x20000, g2_c0=-1), E, b"g2_c0")
    refused(call(N=N, g2=0x20000, g2_c0=C + 1), E, b"g2_c0")
    refused(call(N=N, g2_c0=C + 1), E, b"g2_c0")
    refused(call(N=N, grad_src=[0x100000, 0x10000, 0x300000]), E, b"grad_src[1] is g")
    refused(call(N=N, g2=0x20000, grad_src=[0x100000, 0x200000, 0x20000]), E, b"grad_src[2] is g2")
    refused(call(N=N, grad_src=[0x100000, 0x200000, 0x100000]), E, b"grad_src[2] is grad_src[0]")
    refused(call(N=N, g2=0x10000), E, b"g2 is g")
    refused(call(N=N, grad_src=[None, None, None]), E, b"grad_src")
    # a skipped part is still checked
    refused(call(N=N, grad_src=[None, 0x200000, 0x300000], src_h=[H + 1, 5, 2]), E, b"RC_PART_COPY")


@pytest.mark.parametrize("N", [0, 1])
def test_unsupported_g_layouts(N):
    """Neither planar nor interleaved: RC_EUNSUPPORTED before any launch."""
    U = _lib.RC_EUNSUPPORTED
    C = sum(p[1] for p in PARTS)
    refused(call(N=N, g_strides=(2 * C * H * W, 2 * H * W, 2 * W, 2)), U, b"g_strides")
    refused(call(N=N, g_strides=(C * H * (W + 3), H * (W + 3), W + 3, 1)), U, b"g_strides")
    refused(call(N=N, g_strides=(H * W * C * 2, 2, W * C * 2, C * 2)), U, b"g_strides")


def test_work_to_do_needs_aligned_pointers_and_sizes_under_2_31():
    refused(call(g=0x10001, g_dtype=_lib.RC_BF16), _lib.RC_EINVAL, b"aligned")
    refused(call(g2=0x20001, g_dtype=_lib.RC_BF16), _lib.RC_EINVAL, b"g2")
    refused(call(grad_src=[0x100000, 0x200002, 0x300000]), _lib.RC_EINVAL, b"grad_src[1]")
    big = [(COPY, 1 << 10, 1 << 10, 1 << 10)]
    refused(call(N=4, H=1 << 10, W=1 << 10, parts=big), _lib.RC_EUNSUPPORTED, b"2^31")
    # g is small, the output of a downscale is not
    refused(call(N=1, H=2, W=2, parts=[(BIL, 1 << 11, 1 << 10, 1 << 10)]), _lib.RC_EUNSUPPORTED, b"output")


def test_wrappers_have_no_cpu_fallback():
    g = torch.zeros(1, 6, 3, 5)
    meta = (("copy", (1, 4, 3, 5), torch.float32), ("pool2x", (1, 2, 5, 9), torch.float32))
    with pytest.raises(RuntimeError, match="HIP"):
        gru.assemble_backward(g, meta)
    t = torch.zeros(1, 4, 3, 5, requires_grad=True)
    with pytest.raises(RuntimeError, match="HIP"):
        gru.assemble([t, gru.Pooled(torch.zeros(1, 2, 5, 9))], torch.float32, differentiable=True)
    # the keyword lifts the gradient's refusal only: the device is the reason then
    assert "gradient" in gru.why_not_assemblable([t], torch.float32)
    assert "HIP devices only" in gru.why_not_assemblable([t], torch.float32, differentiable=True)
    with torch.no_grad():
        assert "HIP devices only" in gru.why_not_assemblable([t], torch.float32)


def test_keyword_needs_the_three_options_and_keeps_the_module_tree():
    for missing in ("fuse_gru", "fuse_gru_backward", "fuse_gru_inputs"):
        kw = {k: v for k, v in ALL.items() if k != missing}
        if missing == "fuse_gru":
            kw = {"fuse_gru_inputs_backward": True}     # the others need fuse_gru themselves
        with pytest.raises(ValueError, match="fuse_gru"):
            RAFTStereo(StereoArgs(), **kw)
    with pytest.raises(ValueError, match="fuse_gru_inputs_backward"):
        RAFTStereo(StereoArgs(), fuse_gru=True, fuse_gru_backward=True, fuse_gru_inputs_backward=True)
    with pytest.raises(ValueError, match="fuse_gru_inputs_backward"):
        RAFTStereo(StereoArgs(), fuse_gru=True, fuse_gru_inputs=True, fuse_gru_inputs_backward=True)
    torch.manual_seed(0)
    base = RAFTStereo(StereoArgs())
    torch.manual_seed(0)
    fused = RAFTStereo(StereoArgs(), **ALL)
    assert list(fused.state_dict()) == list(base.state_dict())
    ub = fused.update_block
    assert fused.fuse_gru_inputs_backward and ub.gru08.fuse_inputs_backward and ub.gru16.fuse_inputs_backward \
        and ub.gru32.fuse_inputs_backward
    ub = base.update_block
    assert not (base.fuse_gru_inputs_backward or ub.gru08.fuse_inputs_backward or ub.gru16.fuse_inputs_backward
                or ub.gru32.fuse_inputs_backward)
    three = RAFTStereo(StereoArgs(), fuse_gru=True, fuse_gru_backward=True, fuse_gru_inputs=True)
    assert not three.fuse_gru_inputs_backward and not three.update_block.gru16.fuse_inputs_backward
    assert ConvGRU(8, 8).fuse_inputs_backward is False


def test_cpu_module_takes_the_torch_ops_bit_for_bit():
    """On CPU tensors nothing is fusable: with every attribute set the module
    runs the PyTorch ops, forward and backward."""
    torch.manual_seed(0)
    m = ConvGRU(8, 12).eval()
    g = torch.Generator().manual_seed(1)
    h, cz, cr, cq = (torch.randn(1, 8, 5, 6, generator=g) for _ in range(4))
    a, b = torch.randn(1, 6, 9, 11, generator=g), torch.randn(1, 6, 3, 3, generator=g)

    def step(lazy):
        leaves = [t.clone().requires_grad_(True) for t in (h, cz, cr, cq, a, b)]
        x = (gru.Pooled(leaves[4]), gru.Resized(leaves[5], (5, 6))) if lazy else \
            gru.materialized((gru.Pooled(leaves[4]), gru.Resized(leaves[5], (5, 6))))
        m.zero_grad(set_to_none=True)
        out = m(*leaves[:4], *x)
        out.square().sum().backward()
        return [out.detach()] + [t.grad for t in leaves] + [p.grad.clone() for p in m.parameters()]

    want = step(False)
    m.fuse = m.fuse_backward = m.fuse_inputs = m.fuse_inputs_backward = True
    got = step(True)
    assert all(torch.equal(x, y) for x, y in zip(got, want))


def test_cpu_network_gradients_are_the_default_ones_bit_for_bit():
    g = torch.Generator().manual_seed(8)
    img1 = torch.rand(1, 3, 64, 96, generator=g) * 255
    img2 = torch.roll(img1, -4, dims=-1)
    runs = []
    for kw in ({}, ALL):
        torch.manual_seed(0)
        model = RAFTStereo(StereoArgs(), corr_block=torch_ref.TorchCorrBlock1D, **kw).eval()
        preds = model(img1, img2, iters=2)
        preds[-1][:, 0].abs().mean().backward()
        runs.append(([p.detach() for p in preds], {n: p.grad for n, p in model.named_parameters()
                                                   if p.grad is not None}))
    (p0, g0), (p1, g1) = runs
    assert all(torch.equal(a, b) for a, b in zip(p0, p1))
    assert g0.keys() == g1.keys() and g0
    assert all(torch.equal(g0[n], g1[n]) for n in g0)
