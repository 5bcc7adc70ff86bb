"""rc_gru_assemble_backward on guarded memory (the arena of sweep_util.py),
through the raw C ABI.

Every run carves g, g2 and every output out of one NaN-filled buffer at the
arena's two sub-line phases and checks that the guards and the inputs are
bit-identical afterwards, that every element of every output was written and
that the 8 channels in front of the sliced output still hold the fill.

Cases: those of test_gru_inputs_gpu.py (g N x H x W; parts: mode, channels,
source h x w; a "copy32" part has an fp32 gradient output whatever g is), and
  down   1x3x4    bilinear 4 into 7x9: a downscale; 45 of the 63 source pixels
                  get no contribution and must read +0;
  up3    2x9x20   bilinear 8 into 4x7: a ratio that is not 2.
Each with g planar and interleaved, the outputs of g's class ("same") or of
the other one ("crossed": the one-element path), the last output a channel
slice of a buffer 8 channels wider, in fp32, fp16 and bf16, with g2 absent and
with g2 present and g2_c0 the first part's channels, and once with a skipped
part.

Bounds: the fp32 results against the float64 adjoint (gru_inputs_bwd_ref.py) at
norm_err <= 1e-5 per output, the project's fp32 bound.  Everything else is bit
equality: fp16 / bf16 against ``.to(dtype)`` of the fp32 kernel on the widened
gradients, planar against interleaved, same against crossed, phase against
phase, a copied part against (g + g2) cast, the same-size resize against G.
One adjoint identity on gru16: <assemble(x), G> against <x,
assemble_backward(G)> in float64 from the fp32 kernels' outputs.
"""
import functools

import numpy as np
import pytest
import torch

import gru_inputs_bwd_ref
from golden_util import norm_err
from raft_stereo_amd import _lib
from sweep_util import SENT16, arena
from test_gru_inputs_gpu import CASES, CODE, DT, LAYOUTS, MODE, OTHER, SLICE, VARIANTS, pack, same_bits, strides
from test_gru_inputs_gpu import result as forward_result
from test_gru_inputs_gpu import values as forward_values

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-5
BCASES = dict(CASES)
BCASES["down"] = ((1, 3, 4), (("bilinear", 4, 7, 9),))
BCASES["up3"] = ((2, 9, 20), (("bilinear", 8, 4, 7),))
NAMES = sorted(BCASES)
G2 = [False, True]
G2_IDS = ["g", "g+g2"]


@functools.lru_cache(maxsize=None)
def gradients(name, vdt):
    """(g, g2) as fp32 CPU tensors (N, C, H, W), every value representable in
    ``vdt``; never modified."""
    (N, H, W), parts = BCASES[name]
    C = sum(p[1] for p in parts)
    gen = torch.Generator().manual_seed(1000 + sum(map(ord, name)))
    return tuple(torch.randn(N, C, H, W, generator=gen).to(DT[vdt]).float() for _ in range(2))


def combined(name, vdt, two):
    """G in fp32: g, plus g2 from the first part's channels on."""
    g, g2 = gradients(name, vdt)
    G = g.clone()
    if two:
        c0 = BCASES[name][1][0][1]
        G[:, c0:] = g[:, c0:] + g2[:, c0:]
    return G


def run(name, vdt, kdt, layout, variant, phase, two, skip=None):
    """One rc_gru_assemble_backward call on the case's gradients
    (representable in ``vdt``) as ``kdt`` arrays of ``layout``; the outputs as
    CPU tensors (N, C_i, h_i, w_i), None for the skipped part."""
    (N, H, W), parts = BCASES[name]
    dt = DT[kdt]
    es = 4 if kdt == "fp32" else 2
    g, g2 = gradients(name, vdt)
    C = sum(p[1] for p in parts)
    specs = [("g", g.numel() * es, pack(g.to(dt), layout))]
    if two:
        specs.append(("g2", g.numel() * es, pack(g2.to(dt), layout)))
    meta = []
    for i, (mode, Ci, h, w) in enumerate(parts):
        odt = torch.float32 if mode == "copy32" else dt
        oes = 4 if odt == torch.float32 else 2
        lay = OTHER[layout] if variant == "crossed" else layout
        c0 = SLICE if i == len(parts) - 1 else 0
        if i != skip:
            specs.append((f"o{i}", N * (Ci + c0) * h * w * oes, None))
        meta.append((c0 * (h * w if lay == "planar" else 1) * oes, strides(Ci + c0, h, w, lay), odt, lay, c0))
    ar = arena(DEV, specs, phase, es == 2)
    rc = _lib.lib().rc_gru_assemble_backward(
        ar.ptr("g"), ar.ptr("g2") if two else None, parts[0][1] if two else 0,
        _lib.long_array(strides(C, H, W, layout)), CODE[dt], N, H, W, len(parts),
        _lib.ptr_array([None if i == skip else ar.ptr(f"o{i}") + m[0] for i, m in enumerate(meta)]),
        _lib.long_array([s for m in meta for s in m[1]]), _lib.int_array([CODE[m[2]] for m in meta]),
        _lib.int_array([MODE[p[0]] for p in parts]), _lib.int_array([p[1] for p in parts]),
        _lib.int_array([p[2] for p in parts]), _lib.int_array([p[3] for p in parts]), None)
    _lib.check(rc, "rc_gru_assemble_backward")
    torch.cuda.synchronize()
    ar.assert_guards_intact()
    outs = []
    for i, ((mode, Ci, h, w), (_, _, odt, lay, c0)) in enumerate(zip(parts, meta)):
        if i == skip:
            outs.append(None)
            continue
        wide = odt == torch.float32
        raw = ar.region(f"o{i}", np.uint32 if wide else np.uint16).copy()
        fill = raw == (np.uint32(ar.sent) if wide else np.uint16(SENT16))
        shape = (N, Ci + c0, h, w) if lay == "planar" else (N, h, w, Ci + c0)
        fill = fill.reshape(shape) if lay == "planar" else fill.reshape(shape).transpose(0, 3, 1, 2)
        assert not fill[:, c0:].any(), f"output {i}: {int(fill[:, c0:].sum())} of {fill[:, c0:].size} never written"
        assert fill[:, :c0].all(), f"output {i}: the channels in front of the slice were written"
        flat = torch.from_numpy(raw.view(np.uint8)).view(odt)
        full = flat.view(shape) if lay == "planar" else flat.view(shape).permute(0, 3, 1, 2)
        outs.append(full[:, c0:].contiguous())
    return outs


@functools.lru_cache(maxsize=None)
def result(name, vdt, kdt, layout, variant="same", phase=0, two=False, skip=None):
    """``run``, once per combination for the whole module."""
    return run(name, vdt, kdt, layout, variant, phase, two, skip)


@functools.lru_cache(maxsize=None)
def reference(name, two):
    """The float64 adjoint of the fp32 gradients, per part."""
    parts = [("copy" if p[0] == "copy32" else p[0], *p[1:]) for p in BCASES[name][1]]
    return gru_inputs_bwd_ref.assemble_backward(combined(name, "fp32", two).double().numpy(), parts)


def all_same_bits(got, want, what):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        same_bits(a, b, f"{what}, output {i}")


@pytest.mark.parametrize("phase", [0, 1])
@pytest.mark.parametrize("two", G2, ids=G2_IDS)
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", NAMES)
def test_fp32_values(name, layout, variant, two, phase):
    got = result(name, "fp32", "fp32", layout, variant, phase, two)
    ref = reference(name, two)
    for i, (a, r) in enumerate(zip(got, ref)):
        assert tuple(a.shape) == r.shape and a.dtype == torch.float32
        assert np.isfinite(a.numpy()).all()
        err = norm_err(a.numpy(), r)
        print(f"{name} {layout} {variant} output {i}: norm_err {err:.2e} vs float64")
        assert err <= TOL, (i, err)
    all_same_bits(got, result(name, "fp32", "fp32", layout, variant, 0, two), "phase 1 vs phase 0")


@pytest.mark.parametrize("two", G2, ids=G2_IDS)
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("kdt", ["fp16", "bf16"])
@pytest.mark.parametrize("name", NAMES)
def test_half_is_the_fp32_result_rounded_once(name, kdt, layout, variant, two):
    wide = result(name, kdt, "fp32", layout, variant, 0, two)
    want = [t if p[0] == "copy32" else t.to(DT[kdt]) for t, p in zip(wide, BCASES[name][1])]
    for phase in (0, 1):
        all_same_bits(result(name, kdt, kdt, layout, variant, phase, two), want, f"{kdt} phase {phase} vs fp32.to()")


@pytest.mark.parametrize("two", G2, ids=G2_IDS)
@pytest.mark.parametrize("kdt", list(DT))
@pytest.mark.parametrize("name", NAMES)
def test_layout_classes_agree(name, kdt, two):
    base = result(name, kdt, kdt, "planar", "same", 0, two)
    all_same_bits(result(name, kdt, kdt, "interleaved", "same", 0, two), base, "interleaved vs planar")
    all_same_bits(result(name, kdt, kdt, "planar", "crossed", 0, two), base, "planar g, interleaved outputs")
    all_same_bits(result(name, kdt, kdt, "interleaved", "crossed", 0, two), base, "interleaved g, planar outputs")


@pytest.mark.parametrize("two", G2, ids=G2_IDS)
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("kdt", list(DT))
@pytest.mark.parametrize("name", NAMES)
def test_copies_are_the_gradient_cast(name, kdt, layout, variant, two):
    """A copied part's gradient is (g + g2) cast to its type (g alone below
    g2_c0), and so is that of a resize to the source's own size."""
    (N, H, W), parts = BCASES[name]
    got = result(name, kdt, kdt, layout, variant, 0, two)
    G = combined(name, kdt, two)
    c = 0
    for (mode, C, h, w), a in zip(parts, got):
        if mode in ("copy", "copy32") or (mode == "bilinear" and (h, w) == (H, W)):
            same_bits(a, G[:, c:c + C].to(a.dtype), f"{name} part at channel {c} ({mode})")
        c += C


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("kdt", list(DT))
def test_unread_source_pixels_are_plus_zero(kdt, layout):
    ref, = reference("down", False)
    unread = ref == 0.0
    assert int(unread[0, 0].sum()) == 45 and unread.all(axis=(0, 1)).sum() == 45
    for variant in VARIANTS:
        got, = result("down", kdt, kdt, layout, variant)
        raw = got.contiguous().view(torch.int32 if kdt == "fp32" else torch.int16).numpy()
        assert (raw[unread] == 0).all(), "an unread source pixel is not +0"
        assert (raw[~unread] != 0).all()


@pytest.mark.parametrize("two", G2, ids=G2_IDS)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("kdt", ["fp32", "bf16"])
@pytest.mark.parametrize("name,skip", [("gru16", 1), ("mid", 0), ("wide", 3)])
def test_skipped_part(name, skip, kdt, layout, two):
    """A NULL output: its channels still count, the others are unchanged."""
    full = result(name, kdt, kdt, layout, "same", 0, two)
    got = result(name, kdt, kdt, layout, "same", 0, two, skip)
    assert got[skip] is None
    all_same_bits([t for t in got if t is not None], [t for i, t in enumerate(full) if i != skip], f"skip {skip}")


def test_adjoint_identity():
    """<assemble(x), G> == <x, assemble_backward(G)> in float64, from the fp32
    kernels' outputs on gru16."""
    y = forward_result("gru16", "fp32", "fp32", "planar").double()
    xs = forward_values("gru16", "fp32")
    for two in G2:
        G = combined("gru16", "fp32", two).double()
        grads = result("gru16", "fp32", "fp32", "planar", "same", 0, two)
        lhs = float((y * G).sum())
        rhs = float(sum((x.double() * gx.double()).sum() for x, gx in zip(xs, grads)))
        scale = float(sum((x.double() * gx.double()).abs().sum() for x, gx in zip(xs, grads)))
        print(f"adjoint identity: {lhs:.9e} vs {rhs:.9e}, relative to sum|x g| {abs(lhs - rhs) / scale:.2e}")
        assert abs(lhs - rhs) <= 1e-5 * abs(lhs), (lhs, rhs)
