"""rc_gru_assemble on guarded memory (the arena of sweep_util.py), through the
raw C ABI.

Every run carves its sources and dst out of one NaN-filled buffer at the
arena's two sub-line phases and checks that the guards and every input are
bit-identical afterwards and that every dst element was written.

Cases (dst N x H x W; parts: mode, channels, source H x W), the smallest that
take each path of the kernel (csrc/gru_inputs.hip: 16-byte accesses where
every base, stride and length allows, else 8-byte, else one element):
  tiny   1x3x5    copy 8; pool 3 from 5x9; bilinear 5 from 2x3: H*W under one
                  wave, odd channel counts, one element per access everywhere;
  mid    2x5x13   copy 16; pool 16 from 10x26 (even source); pool 8 from 9x25
                  (odd source); bilinear 24 from 3x7: interleaved 16 bytes,
                  planar one element;
  gru16  2x9x20   copy 128; pool 128 from 17x39; bilinear 128 from 5x10;
  gru08  2x9x20   copy 128; copy 128 from an fp32 source (the motion features
                  under autocast); bilinear 128 from 5x10: several workgroups
                  with a partial last one; planar 16 bytes in fp32, 8 in fp16 /
                  bf16 (20 % 8 = 4);
  row    1x1x8    bilinear 4 from 1x4 and from 1x1; pool 4 from 1x15: D == 1
                  (scale 0) along H, a 1-pixel source; planar 16 bytes in
                  fp16 / bf16 with gathered parts;
  col    1x4x1    bilinear 4 from 1x1 and from 3x1; pool 4 from 7x1;
  same   1x3x5    bilinear 8 from 3x5: the source's bits;
  wide   1x2x16   copy 4; copy 4 from fp32; pool 4 from 3x31; bilinear 4 from
                  2x5: planar 16 bytes in fp16 / bf16 with copied parts;
  w6     1x2x6    copy 2; pool 2 from 3x11; bilinear 2 from 2x2: 8 bytes in
                  fp32, planar and interleaved.
Each with dst planar and interleaved, the sources of dst's class ("same") or
every source but h of the other class ("crossed"), the last part a channel
slice of a buffer 8 channels wider, in fp32, fp16 and bf16.

Bounds: the fp32 results against the float64 evaluation (gru_inputs_ref.py)
and against F.avg_pool2d / F.interpolate / torch.cat on the device at
norm_err <= 1e-5, the project's fp32 bound (TOL of test_gru_network_gpu.py);
how many elements differ in bits from the torch ops is printed, not asserted.
Everything else is bit equality: fp16 / bf16 against ``.to(dtype)`` of the
fp32 kernel on the widened inputs, planar against interleaved, same against
crossed, phase against phase, copied parts and the same-size resize against
their sources.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gru_inputs_ref
from golden_util import norm_err
from raft_stereo_amd import _lib
from sweep_util import arena

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-5
CASES = {
    "tiny": ((1, 3, 5), (("copy", 8, 3, 5), ("pool", 3, 5, 9), ("bilinear", 5, 2, 3))),
    "mid": ((2, 5, 13), (("copy", 16, 5, 13), ("pool", 16, 10, 26), ("pool", 8, 9, 25), ("bilinear", 24, 3, 7))),
    "gru16": ((2, 9, 20), (("copy", 128, 9, 20), ("pool", 128, 17, 39), ("bilinear", 128, 5, 10))),
    "gru08": ((2, 9, 20), (("copy", 128, 9, 20), ("copy32", 128, 9, 20), ("bilinear", 128, 5, 10))),
    "row": ((1, 1, 8), (("bilinear", 4, 1, 4), ("bilinear", 4, 1, 1), ("pool", 4, 1, 15))),
    "col": ((1, 4, 1), (("bilinear", 4, 1, 1), ("bilinear", 4, 3, 1), ("pool", 4, 7, 1))),
    "same": ((1, 3, 5), (("bilinear", 8, 3, 5),)),
    "wide": ((1, 2, 16), (("copy", 4, 2, 16), ("copy32", 4, 2, 16), ("pool", 4, 3, 31), ("bilinear", 4, 2, 5))),
    "w6": ((1, 2, 6), (("copy", 2, 2, 6), ("pool", 2, 3, 11), ("bilinear", 2, 2, 2))),
}
NAMES = sorted(CASES)
DT = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
CODE = {torch.float32: _lib.RC_F32, torch.float16: _lib.RC_F16, torch.bfloat16: _lib.RC_BF16}
MODE = {"copy": _lib.RC_PART_COPY, "copy32": _lib.RC_PART_COPY, "pool": _lib.RC_PART_POOL2X,
        "bilinear": _lib.RC_PART_BILINEAR}
LAYOUTS = ["planar", "interleaved"]
VARIANTS = ["same", "crossed"]
OTHER = {"planar": "interleaved", "interleaved": "planar"}
SLICE = 8           # the last part sits behind 8 more channels of its buffer


@functools.lru_cache(maxsize=None)
def values(name, vdt):
    """One fp32 CPU tensor (N, C, h, w) per part, every value representable in
    ``vdt`` (a "copy32" part keeps its fp32 values: its source is fp32 whatever
    dst is); never modified."""
    (N, _, _), parts = CASES[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    out = []
    for mode, C, h, w in parts:
        t = torch.randn(N, C, h, w, generator=g)
        out.append(t if mode == "copy32" else t.to(DT[vdt]).float())
    return tuple(out)


def pack(t, layout):
    """(N, K, h, w) -> the memory of that layout: as it is, or (N, h, w, K)."""
    return t.contiguous() if layout == "planar" else t.permute(0, 2, 3, 1).contiguous()


def strides(K, h, w, layout):
    return (K * h * w, h * w, w, 1) if layout == "planar" else (h * w * K, 1, w * K, K)


def run(name, vdt, kdt, layout, variant, phase):
    """One rc_gru_assemble call on the case's values (representable in
    ``vdt``) with a ``kdt`` dst of ``layout``; the filled dst as a CPU tensor
    (N, C, H, W)."""
    (N, H, W), parts = CASES[name]
    dt = DT[kdt]
    es = 4 if kdt == "fp32" else 2
    vals = values(name, vdt)
    C = sum(p[1] for p in parts)
    specs, meta = [], []
    for i, ((mode, Ci, h, w), v) in enumerate(zip(parts, vals)):
        sdt = torch.float32 if mode == "copy32" else dt
        lay = OTHER[layout] if variant == "crossed" and i > 0 else layout
        c0 = SLICE if i == len(parts) - 1 else 0
        g = torch.Generator().manual_seed(i)
        full = torch.cat([torch.randn(N, c0, h, w, generator=g), v], 1) if c0 else v
        mem = pack(full.to(sdt), lay)
        specs.append((f"s{i}", mem.numel() * mem.element_size(), mem))
        off = c0 * (h * w if lay == "planar" else 1) * mem.element_size()
        meta.append((off, strides(Ci + c0, h, w, lay), CODE[sdt]))
    specs.append(("dst", N * C * H * W * es, None))
    ar = arena(DEV, specs, phase, es == 2)
    rc = _lib.lib().rc_gru_assemble(
        ar.ptr("dst"), _lib.long_array(strides(C, H, W, layout)), CODE[dt], N, H, W, len(parts),
        _lib.ptr_array([ar.ptr(f"s{i}") + m[0] for i, m in enumerate(meta)]),
        _lib.long_array([s for m in meta for s in m[1]]), _lib.int_array([m[2] for m in meta]),
        _lib.int_array([MODE[p[0]] for p in parts]), _lib.int_array([p[1] for p in parts]),
        _lib.int_array([p[2] for p in parts]), _lib.int_array([p[3] for p in parts]), None)
    _lib.check(rc, "rc_gru_assemble")
    torch.cuda.synchronize()
    ar.assert_guards_intact()
    ar.assert_outputs_written(["dst"], es)
    flat = torch.from_numpy(ar.region("dst", np.uint8).copy()).view(dt)
    out = flat.view(N, C, H, W) if layout == "planar" else flat.view(N, H, W, C).permute(0, 3, 1, 2)
    return out.contiguous()


@functools.lru_cache(maxsize=None)
def result(name, vdt, kdt, layout, variant="same", phase=0):
    """``run``, once per combination for the whole module."""
    return run(name, vdt, kdt, layout, variant, phase)


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def same_bits(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, what
    assert torch.equal(bits(a), bits(b)), \
        f"{what}: {int((bits(a) != bits(b)).sum())} of {a.numel()} elements differ"


@functools.lru_cache(maxsize=None)
def references(name):
    """(float64 evaluation, the torch ops on the device) of the fp32 values."""
    (N, H, W), parts = CASES[name]
    vals = values(name, "fp32")
    key = {"copy": "copy", "copy32": "copy", "pool": "pool", "bilinear": "bilinear"}
    ref64 = gru_inputs_ref.assemble([(key[p[0]], v.numpy()) for p, v in zip(parts, vals)], H, W)
    outs = []
    for (mode, _, _, _), v in zip(parts, vals):
        d = v.to(DEV)
        if mode == "pool":
            d = F.avg_pool2d(d, 3, stride=2, padding=1)
        elif mode == "bilinear":
            d = F.interpolate(d, (H, W), mode="bilinear", align_corners=True)
        outs.append(d)
    return ref64, torch.cat(outs, 1).cpu()


@pytest.mark.parametrize("phase", [0, 1])
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", NAMES)
def test_fp32_values(name, layout, variant, phase):
    got = result(name, "fp32", "fp32", layout, variant, phase)
    ref64, ref_torch = references(name)
    assert tuple(got.shape) == ref64.shape == tuple(ref_torch.shape)
    e64, et = norm_err(got.numpy(), ref64), norm_err(got.numpy(), ref_torch.numpy())
    differ = int((bits(got) != bits(ref_torch)).sum())
    print(f"{name} {layout} {variant}: norm_err {e64:.2e} vs float64, {et:.2e} vs the torch ops; "
          f"{differ} of {got.numel()} elements differ in bits from the torch ops")
    assert np.isfinite(got.numpy()).all()
    assert e64 <= TOL and et <= TOL, (e64, et)
    same_bits(got, result(name, "fp32", "fp32", layout, variant, 0), "phase 1 vs phase 0")


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("kdt", ["fp16", "bf16"])
@pytest.mark.parametrize("name", NAMES)
def test_half_is_the_fp32_result_rounded_once(name, kdt, layout, variant):
    want = result(name, kdt, "fp32", layout, variant).to(DT[kdt])
    for phase in (0, 1):
        same_bits(result(name, kdt, kdt, layout, variant, phase), want, f"{kdt} phase {phase} vs fp32.to()")


@pytest.mark.parametrize("kdt", list(DT))
@pytest.mark.parametrize("name", NAMES)
def test_layout_classes_agree(name, kdt):
    base = result(name, kdt, kdt, "planar", "same")
    same_bits(result(name, kdt, kdt, "interleaved", "same"), base, "interleaved vs planar")
    same_bits(result(name, kdt, kdt, "planar", "crossed"), base, "planar dst, interleaved sources")
    same_bits(result(name, kdt, kdt, "interleaved", "crossed"), base, "interleaved dst, planar sources")


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("kdt", list(DT))
@pytest.mark.parametrize("name", NAMES)
def test_copies_keep_the_source_bits(name, kdt, layout, variant):
    """A copied part is the source's bits (an fp32 source of a 16-bit dst: its
    ``.to(dtype)``), and so is a resize to the source's own size."""
    (N, H, W), parts = CASES[name]
    got = result(name, kdt, kdt, layout, variant)
    c = 0
    for (mode, C, h, w), v in zip(parts, values(name, kdt)):
        if mode in ("copy", "copy32") or (mode == "bilinear" and (h, w) == (H, W)):
            same_bits(got[:, c:c + C], v.to(DT[kdt]), f"{name} part at channel {c} ({mode})")
        c += C
