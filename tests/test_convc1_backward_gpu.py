"""Backward of the fused lookup + convc1 (rc_corr_lookup_conv_backward,
``CorrBlock1D.lookup_convc1(..., differentiable=True)``).

Reference: fp64 CPU autograd of ``relu(conv2d(TorchCorrBlock1D(f1, f2, L, r)
(coords), W, b))`` contracted with a random ``grad_out`` (oracle.torch_ref; its
lookup result is rounded to fp32 once, 6e-8 relative, before the fp64 conv).
Bound: the project's fp32 bound, norm_err <= 1e-5, raised to 4 x the error of
the same reference evaluated in fp32 on the CPU where that exceeds 2.5e-6 (the
sampler's fp32 coordinate round trip is part of both).

ReLU kink: a pre-activation within rounding of zero may land on either side,
so ``grad_out`` is zeroed where |pre| of the fp64 reference is below
1e-4 max|pre| -- decided from the reference alone, at most 0.1 % of the
entries (asserted).  Non-finite pre-activations (NaN / inf coords) have no
defined ReLU derivative (PyTorch passes the gradient through a NaN, the kernel
masks with ``pre > 0``): ``grad_out`` is zeroed there as well, again from the
reference alone, and counted separately.

Largest errors measured on MI355X are recorded in DESIGN.md §3.2b."""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from golden_util import norm_err
from oracle.torch_ref import TorchCorrBlock1D
from raft_stereo_amd import CorrBlock1D, _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5

SHAPES = [
    # B, D, H, W1, W2, L, r, cout
    (1, 8, 1, 20, 16, 4, 1, 8),       # P = 20 < one wave; level 3 of width 2
    (2, 16, 3, 57, 240, 4, 4, 64),    # P = 342: two workgroups, the second partial; W1 != W2
    (3, 8, 2, 130, 129, 3, 3, 63),    # P = 780: four workgroups; odd cout and widths
    (1, 8, 2, 33, 64, 2, 2, 1),       # cout = 1, two levels
    (2, 64, 5, 96, 96, 4, 4, 64),     # the forward test's shape (also with a bf16 pyramid)
]
IDS = ["x".join(map(str, s)) for s in SHAPES]
FOUR_WG = SHAPES[2]
NAMES = ("dW", "db", "df1", "df2")


@functools.lru_cache(maxsize=None)
def inputs(shape, special=False, bias=True):
    """CPU fp32 inputs; grad_out already zeroed at the reference's ReLU kinks
    and non-finite pre-activations (module docstring)."""
    B, D, H, W1, W2, L, r, cout = shape
    g = torch.Generator().manual_seed(100 + sum(shape))
    cin = L * (2 * r + 1)
    f1 = torch.randn(B, D, H, W1, generator=g)
    f2 = torch.randn(B, D, H, W2, generator=g)
    x = torch.arange(W1).float().view(1, 1, 1, W1) - torch.rand(B, 1, H, W1, generator=g) * 30
    x[..., ::7] = torch.rand(x[..., ::7].shape, generator=g) * (W2 + 40) - 20   # zero-padded taps
    if special:
        flat = x.view(-1)
        for i, v in zip((3, 70, 141, 212, 300), (float("nan"), float("inf"), -float("inf"), 1e30, -1e30)):
            flat[i] = v
    coords = torch.cat([x, torch.zeros_like(x)], 1)
    W = torch.randn(cout, cin, generator=g) / cin ** 0.5
    b = torch.randn(cout, generator=g) * 0.1 if bias else None
    gout = torch.randn(B, cout, H, W1, generator=g)
    with torch.no_grad():
        corr = TorchCorrBlock1D(f1.double(), f2.double(), L, r)(coords.double()).double()
        pre = F.conv2d(corr, W.double().view(cout, cin, 1, 1), None if b is None else b.double())
    fin = torch.isfinite(pre)
    kink = fin & (pre.abs() < 1e-4 * pre[fin].abs().max())
    assert kink.float().mean().item() <= 1e-3, "kink mask touched more than 0.1 % of grad_out"
    assert special or bool(fin.all())
    gout[kink | ~fin] = 0.0
    return dict(f1=f1, f2=f2, coords=coords, W=W, b=b, gout=gout, shape=shape,
                kinks=int(kink.sum()), nonfinite=int((~fin).sum()))


@functools.lru_cache(maxsize=None)
def cpu_grads(shape, special, bias, relu, dtype):
    """(dW, db, df1, df2) of the reference in ``dtype`` on the CPU."""
    inp = inputs(shape, special, bias)
    B, D, H, W1, W2, L, r, cout = shape
    cin = L * (2 * r + 1)
    leaf = lambda t: t.detach().clone().to(dtype).requires_grad_(True)  # noqa: E731  (never the cached tensor)
    W, f1, f2 = leaf(inp["W"]), leaf(inp["f1"]), leaf(inp["f2"])
    b = leaf(inp["b"]) if bias else None
    corr = TorchCorrBlock1D(f1, f2, L, r)(inp["coords"].to(dtype)).to(dtype)
    out = F.conv2d(corr, W.view(cout, cin, 1, 1), b)
    if relu:
        out = torch.relu(out)
    out.backward(inp["gout"].to(dtype))
    return (W.grad.numpy(), b.grad.numpy() if bias else None, f1.grad.numpy(), f2.grad.numpy())


def hip_grads(inp, relu=True, fused=True, pyramid_dtype=None, need_w=True, need_f=True, coords=None):
    """(dW, db, df1, df2) on the GPU, through ``lookup_convc1(differentiable=True)``
    (``fused``) or the unfused ``conv2d(blk(coords))`` under autograd."""
    B, D, H, W1, W2, L, r, cout = inp["shape"]
    f1 = inp["f1"].to(DEV).requires_grad_(need_f)
    f2 = inp["f2"].to(DEV).requires_grad_(need_f)
    W = inp["W"].to(DEV).view(cout, -1, 1, 1).requires_grad_(need_w)
    b = inp["b"].to(DEV).requires_grad_(need_w) if inp["b"] is not None else None
    blk = CorrBlock1D(f1, f2, num_levels=L, radius=r, pyramid_dtype=pyramid_dtype)
    c = inp["coords"].to(DEV)
    if fused:
        out = blk.lookup_convc1(c, W, b, relu=relu, differentiable=True)
    else:
        out = F.conv2d(blk(c), W, b)
        out = torch.relu(out) if relu else out
    out.backward(inp["gout"].to(DEV))
    cpu = lambda t: None if t is None or t.grad is None else t.grad.cpu()  # noqa: E731
    gw = cpu(W)
    return (gw.view(cout, -1) if gw is not None else None, cpu(b), cpu(f1), cpu(f2))


def finite_err(got, ref):
    """norm_err over the reference's finite entries (None: there is none)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    fin = np.isfinite(ref)
    if not fin.any():
        return None
    return norm_err(got[fin], ref[fin])


PARITY = ([(s, True, True, False) for s in SHAPES] +
          [(s, bias, relu, False) for s in (SHAPES[1], SHAPES[4])
           for bias, relu in ((False, True), (True, False), (False, False))] +
          [(SHAPES[1], True, True, True)])


@pytest.mark.parametrize("shape,bias,relu,special", PARITY,
                         ids=[f"{'x'.join(map(str, s))}-b{int(b)}-r{int(r)}{'-special' if sp else ''}"
                              for s, b, r, sp in PARITY])
def test_parity_fp32(shape, bias, relu, special):
    inp = inputs(shape, special, bias)
    ref = cpu_grads(shape, special, bias, relu, torch.float64)
    ref32 = cpu_grads(shape, special, bias, relu, torch.float32)
    got = hip_grads(inp, relu)
    if special:
        other = hip_grads(inp, relu, fused=False)
    for i, name in enumerate(NAMES):
        if ref[i] is None:
            assert got[i] is None
            continue
        e32 = finite_err(ref32[i], ref[i])
        e = finite_err(got[i].numpy(), ref[i])
        if e is None:
            print(f"{shape} {name}: no finite reference entry")
        else:
            bound = max(TOL, 4 * e32)
            print(f"{shape} bias={bias} relu={relu} {name}: {e:.2e} (fp32 CPU {e32:.2e}, bound {bound:.2e}; "
                  f"kinks {inp['kinks']}, non-finite {inp['nonfinite']})")
            assert e <= bound, (name, e, bound)
        if special:
            assert torch.equal(torch.isnan(got[i]), torch.isnan(other[i].view_as(got[i]))), name


@pytest.mark.parametrize("pyramid_dtype,shape", [(torch.bfloat16, SHAPES[4]), (None, SHAPES[1])],
                         ids=["bf16", "fp32"])
def test_matches_unfused_gpu_path(pyramid_dtype, shape):
    """Fused vs ``conv2d(blk(coords))`` under autograd on the same pyramid
    (bf16 or fp32): both read the same levels, only summation order differs."""
    inp = inputs(shape)
    got = hip_grads(inp, pyramid_dtype=pyramid_dtype)
    ref = hip_grads(inp, fused=False, pyramid_dtype=pyramid_dtype)
    for name, a, b in zip(NAMES, got, ref):
        e = norm_err(a.numpy(), b.numpy())
        print(f"{shape} {pyramid_dtype} {name}: {e:.2e}")
        assert e <= TOL, (name, e)


def test_needs_input_grad():
    inp = inputs(SHAPES[1])
    both = hip_grads(inp)
    w_only = hip_grads(inp, need_f=False)
    f_only = hip_grads(inp, need_w=False)
    assert w_only[2] is None and w_only[3] is None
    assert f_only[0] is None and f_only[1] is None
    assert torch.equal(w_only[0], both[0]) and torch.equal(w_only[1], both[1])
    assert torch.equal(f_only[2], both[2]) and torch.equal(f_only[3], both[3])


def test_deterministic():
    inp = inputs(FOUR_WG)
    a, b = hip_grads(inp), hip_grads(inp)
    for name, x, y in zip(NAMES, a, b):
        assert torch.equal(x, y), name


def test_several_calls_on_one_block():
    """Three fused calls at different coords plus one plain lookup on one
    block: d fmaps equal the all-unfused graph's, dW accumulates."""
    inp = inputs(SHAPES[1])
    B, D, H, W1, W2, L, r, cout = inp["shape"]
    g = torch.Generator().manual_seed(7)
    shifts = [0.0, -3.25, 5.5, -8.125]
    gouts = [torch.randn(B, cout, H, W1, generator=g).to(DEV) for _ in range(3)]
    gplain = torch.randn(B, L * (2 * r + 1), H, W1, generator=g).to(DEV)

    def run(fused):
        f1 = inp["f1"].to(DEV).requires_grad_(True)
        f2 = inp["f2"].to(DEV).requires_grad_(True)
        W = inp["W"].to(DEV).view(cout, -1, 1, 1).requires_grad_(True)
        b = inp["b"].to(DEV).requires_grad_(True)
        blk = CorrBlock1D(f1, f2, num_levels=L, radius=r)
        loss = 0.0
        for s, go in zip(shifts[:3], gouts):
            c = inp["coords"].to(DEV) + s
            out = (blk.lookup_convc1(c, W, b, differentiable=True) if fused
                   else torch.relu(F.conv2d(blk(c), W, b)))
            loss = loss + (out * go).sum()
        loss = loss + (blk(inp["coords"].to(DEV) + shifts[3]) * gplain).sum()
        loss.backward()
        return [t.grad.cpu().numpy() for t in (W, b, f1, f2)]

    got, ref = run(True), run(False)
    for name, a, b in zip(NAMES, got, ref):
        e = norm_err(a, b)
        print(f"several calls {name}: {e:.2e}")
        assert e <= TOL, (name, e)


def test_no_stored_correlation():
    B, D, H, W1, W2, L, r, cout = SHAPES[4]
    inp = inputs(SHAPES[4])
    cin = L * (2 * r + 1)
    f1 = inp["f1"].to(DEV).requires_grad_(True)
    f2 = inp["f2"].to(DEV).requires_grad_(True)
    W = inp["W"].to(DEV).view(cout, cin, 1, 1).requires_grad_(True)
    b = inp["b"].to(DEV).requires_grad_(True)
    c = inp["coords"].to(DEV)
    blk = CorrBlock1D(f1, f2, num_levels=L, radius=r)
    blk.lookup_convc1(c, W, b, differentiable=True)       # warm-up: lazily pooled levels, library load
    torch.relu(F.conv2d(blk(c), W, b))
    out_bytes = B * cout * H * W1 * 4
    torch.cuda.synchronize()
    m0 = torch.cuda.memory_allocated()
    out = blk.lookup_convc1(c, W, b, differentiable=True)
    torch.cuda.synchronize()
    grown = torch.cuda.memory_allocated() - m0
    assert out.grad_fn is not None
    assert grown <= out_bytes + 64 * 1024, (grown, out_bytes)
    del out
    m0 = torch.cuda.memory_allocated()
    out = torch.relu(F.conv2d(blk(c), W, b))
    torch.cuda.synchronize()
    grown_unfused = torch.cuda.memory_allocated() - m0
    assert grown_unfused >= out_bytes + B * cin * H * W1 * 4, (grown_unfused, out_bytes)
    print(f"allocated: fused {grown} B, unfused {grown_unfused} B (output {out_bytes} B)")


def test_opt_in_and_refusals():
    f = torch.randn(1, 8, 2, 16, device=DEV)
    fg = f.clone().requires_grad_(True)
    conv = torch.nn.Conv2d(18, 8, 1).to(DEV)
    c = torch.zeros(1, 2, 2, 16, device=DEV)
    with pytest.raises(RuntimeError, match="inference-only"):
        CorrBlock1D(fg, fg, num_levels=2, radius=4).lookup_convc1(c, conv.weight, conv.bias)
    with pytest.raises(RuntimeError, match="inference-only"):
        CorrBlock1D(f, f, num_levels=2, radius=4).lookup_convc1(c, conv.weight, conv.bias)
    # grad disabled: differentiable=True is the plain forward
    with torch.no_grad():
        blk = CorrBlock1D(f, f, num_levels=2, radius=4)
        a = blk.lookup_convc1(c, conv.weight, conv.bias, differentiable=True)
        assert a.grad_fn is None and torch.equal(a, blk.lookup_convc1(c, conv.weight, conv.bias))
    # the other layouts keep refusing, whichever value differentiable has
    f1 = torch.randn(1, 256, 2, 128, device=DEV)
    conv36 = torch.nn.Conv2d(36, 8, 1).to(DEV)
    c128 = torch.zeros(1, 2, 2, 128, device=DEV)
    for layout, fm in (("disparity", f1), ("records", f1.bfloat16())):
        with torch.no_grad():
            blk = CorrBlock1D(fm, fm, num_levels=4, radius=4, layout=layout)
        assert blk.layout == layout
        for diff in (False, True):
            with pytest.raises(RuntimeError, match="not available with layout"):
                with torch.no_grad():
                    blk.lookup_convc1(c128, conv36.weight, conv36.bias, differentiable=diff)
        with pytest.raises(RuntimeError, match="not available with layout"):
            blk.lookup_convc1(c128, conv36.weight.detach(), conv36.bias.detach(), differentiable=True)


def test_capi_validation():
    L = _lib.lib()
    p = ctypes.c_void_p
    pyr = _lib.ptr_array([0x10000, 0x20000])
    widths, lds = _lib.int_array([16, 8]), _lib.long_array([16, 8])

    def call(B, gc, gw, gb, ws, levels=2, radius=2, dt=_lib.RC_F32):
        return L.rc_corr_lookup_conv_backward(pyr, widths, lds, dt, levels, radius, p(0x1000), 32, B, 2, 16,
                                              p(0x2000), p(0x3000), 8, 1, p(0x4000), gc, gw, gb, ws, None)

    assert call(1, None, None, None, p(0x8000)) == _lib.RC_EINVAL              # nothing requested
    assert L.rc_last_error()
    assert call(1, p(0x5000), p(0x6000), None, None) == _lib.RC_EINVAL         # grad_weight without workspace
    assert b"workspace" in L.rc_last_error()
    assert call(1, None, None, p(0x7000), None) == _lib.RC_EINVAL              # grad_bias without workspace
    assert call(1, p(0x5000), None, None, None, levels=1) == _lib.RC_EUNSUPPORTED
    assert call(1, p(0x5000), None, None, None, dt=_lib.RC_LAYOUT_RECORDS | _lib.RC_BF16) == _lib.RC_EUNSUPPORTED
    assert call(1, p(0x5000), None, None, None, dt=_lib.RC_OUT_CHANNELS_LAST) == _lib.RC_EUNSUPPORTED
    assert _lib.lookup_conv_bwd_ws(257, 8, 10) == 2 * 8 * 11
    # B*H*W1 == 0: zeros in grad_weight / grad_bias, nothing launched
    gw = torch.full((8, 10), 7.0, device=DEV)
    gb = torch.full((8,), 7.0, device=DEV)
    assert call(0, None, p(gw.data_ptr()), p(gb.data_ptr()), None) == _lib.RC_OK
    torch.cuda.synchronize()
    assert not gw.any() and not gb.any()


def test_network_trains_with_fused_convc1():
    """RAFTStereo(fuse_convc1=True) under grad against its unfused twin, both
    measured against an fp64 CPU run of the same network with the oracle's
    corr block: e_fused <= max(2 e_unfused, 1e-5) for the gradients of
    convc1.weight, convc1.bias and conv2[1].weight (reached only through the
    corr path).  The unfused GPU path is the yardstick; the factor 2 allows for
    the conv's different summation order through three GRU iterations."""
    from oracle import torch_ref
    from raft_stereo_amd import upsample as rup
    from raft_stereo_amd.network import RAFTStereo, StereoArgs

    g = torch.Generator().manual_seed(8)
    img1 = torch.rand(1, 3, 64, 96, generator=g) * 255
    img2 = torch.roll(img1, -4, dims=-1)
    torch.manual_seed(0)
    twin = RAFTStereo(StereoArgs()).eval()
    state = twin.state_dict()
    picks = ("update_block.encoder.convc1.weight", "update_block.encoder.convc1.bias", "conv2.1.weight")

    def grads(model, a, b):
        model.zero_grad()
        preds = model(a, b, iters=3, upsample=True)
        sum(preds).abs().mean().backward()
        named = dict(model.named_parameters())
        return [named[k].grad.detach().double().cpu().numpy() for k in picks]

    class Ref64(TorchCorrBlock1D):       # the oracle block ends in .float()
        def __call__(self, coords):
            return super().__call__(coords).double()

    class RefNet(RAFTStereo):            # fp64 coordinate grids (delta_flow.float() stays, as on the GPU)
        def initialize_flow(self, img):
            c0, c1 = super().initialize_flow(img)
            return c0.double(), c1.double()

    ref_model = RefNet(StereoArgs(), corr_block=Ref64).eval()
    ref_model.load_state_dict(state)
    ref_model = ref_model.double()
    hip_upsample = rup.convex_upsample
    rup.convex_upsample = lambda flow, mask, factor, differentiable=False: \
        torch_ref.convex_upsample(flow, mask, factor)
    try:
        ref = grads(ref_model, img1.double(), img2.double())
    finally:
        rup.convex_upsample = hip_upsample

    errs = {}
    for fuse in (False, True):
        model = RAFTStereo(StereoArgs(), fuse_convc1=fuse).eval()
        model.load_state_dict(state)
        model = model.cuda()
        got = grads(model, img1.cuda(), img2.cuda())
        errs[fuse] = [norm_err(a, r) for a, r in zip(got, ref)]
    for k, eu, ef in zip(picks, errs[False], errs[True]):
        print(f"{k}: unfused {eu:.2e}, fused {ef:.2e}")
    for k, eu, ef in zip(picks, errs[False], errs[True]):
        assert ef <= max(2 * eu, TOL), (k, ef, eu)
