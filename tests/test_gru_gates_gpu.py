"""rc_gru_gates / rc_gru_blend on guarded memory (the arena of sweep_util.py),
through the raw C ABI.

Every run carves its operands out of one NaN-filled buffer at the arena's two
sub-line phases and checks that the guards and the inputs are bit-identical
afterwards, that every output element was written, and that the x channels
behind the r*h channels of the [r*h, x] buffer keep their bits.

Shapes (N, C, Cx, H, W), the smallest that take each path of the kernels
(csrc/gru_gates.hip: 16-byte accesses where every base, stride and the
unit-stride length allow, else 8-byte, else one element):
  (1, 8, 3, 3, 5)      H*W = 15, under one wave; planar rows at 2- / 4-byte
                       aligned bases and an interleaved pixel stride of
                       C + Cx = 11: one element per access everywhere;
  (2, 16, 24, 5, 13)   H*W = 65: planar one element, interleaved 16 bytes,
                       batch strides of channel slices;
  (2, 128, 256, 9, 20) gru08's channel counts, several workgroups with a
                       partial last one; planar 16 bytes in fp32 and 8 bytes
                       in fp16 / bf16 (180 % 8 = 4), interleaved 16 bytes;
  (1, 6, 4, 2, 8)      planar 16 bytes in every dtype; interleaved strides
                       6, 10, 12, 18: 8 bytes in fp32, one element in 16 bits.
Each in the planar and the interleaved layout class, with z_pre / r_pre as the
halves of one stacked buffer or as two, cz / cr / cq as thirds of one buffer,
in fp32, fp16 and bf16.

Bounds: the fp32 results against the float64 evaluation (gru_ref.py) and
against the torch fp32 op sequence at norm_err <= 1e-5, the project's fp32
bound (TOL of test_pair_convc1_gpu.py).  Everything else is bit equality:
fp16 / bf16 against ``.to(dtype)`` of the fp32 kernel on the widened inputs,
planar against interleaved, in place against out of place, phase against
phase.
"""
import functools

import numpy as np
import pytest
import torch

import gru_ref
from golden_util import norm_err
from raft_stereo_amd import _lib
from sweep_util import SENT16, SENT32, arena

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-5
SHAPES = [(1, 8, 3, 3, 5), (2, 16, 24, 5, 13), (2, 128, 256, 9, 20), (1, 6, 4, 2, 8)]
SHAPE_IDS = ["x".join(map(str, s)) for s in SHAPES]
DT = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
CODE = {"fp32": _lib.RC_F32, "fp16": _lib.RC_F16, "bf16": _lib.RC_BF16}
LAYOUTS = ["planar", "interleaved"]
NAMES = ("z_pre", "r_pre", "cz", "cr", "cq", "h", "q_pre", "z", "x")


@functools.lru_cache(maxsize=None)
def values(shape, vdt):
    """fp32 CPU tensors (N, channels, H*W), every value representable in
    ``vdt``; never modified."""
    N, C, Cx, H, W = shape
    g = torch.Generator().manual_seed(sum(shape))
    v = {k: torch.randn(N, C, H * W, generator=g) * s
         for k, s in (("z_pre", 2.0), ("r_pre", 2.0), ("q_pre", 2.0), ("cz", 1.0), ("cr", 1.0), ("cq", 1.0))}
    v["h"] = torch.tanh(torch.randn(N, C, H * W, generator=g))
    v["z"] = torch.rand(N, C, H * W, generator=g)
    v["x"] = torch.randn(N, Cx, H * W, generator=g)
    return {k: t.to(DT[vdt]).float() for k, t in v.items()}


def pack(t, layout):
    """(N, K, HW) -> the buffer of that layout: as it is, or (N, HW, K)."""
    return t.contiguous() if layout == "planar" else t.permute(0, 2, 1).contiguous()


def unpack(flat, N, K, HW, layout):
    return flat.view(N, K, HW) if layout == "planar" else flat.view(N, HW, K).permute(0, 2, 1)


def view(ar, name, K, c0, shape, layout, es):
    """(address, stride triple) of channels [c0, c0 + C) of the K-channel buffer ``name``."""
    HW = shape[3] * shape[4]
    if layout == "planar":
        return ar.ptr(name) + c0 * HW * es, (K * HW, HW, 1)
    return ar.ptr(name) + c0 * es, (HW * K, 1, K)


def sentinel(n, dt):
    if dt == torch.float32:
        return torch.full((n,), SENT32, dtype=torch.int32).view(torch.float32)
    return torch.full((n,), SENT16, dtype=torch.int16).view(dt)


def run(v, shape, kdt, layout, stacked=True, inplace=False, phase=0):
    """Both kernels on the values ``v`` in dtype ``kdt``; returns z, r*h and
    h_out as CPU tensors (N, C, HW) of that dtype."""
    N, C, Cx, H, W = shape
    HW = H * W
    dt, code = DT[kdt], CODE[kdt]
    es = 4 if kdt == "fp32" else 2
    half = es == 2

    def buf(*names):
        return pack(torch.cat([v[k] for k in names], 1).to(dt), layout)

    def spec(name, t, inout=False):
        return (name, t.numel() * es, t, inout)

    def fetch(ar, name, K, c0=0):
        flat = torch.from_numpy(ar.region(name, np.uint8).copy()).view(dt)
        return unpack(flat, N, K, HW, layout)[:, c0:c0 + C].contiguous()

    # ---- gates
    hx0 = pack(torch.cat([sentinel(N * C * HW, dt).view(N, C, HW), v["x"].to(dt)], 1), layout)
    specs = [spec("zr", buf("z_pre", "r_pre"), inplace)] if stacked else \
        [spec("zp", buf("z_pre"), inplace), spec("rp", buf("r_pre"))]
    specs += [spec("ctx", buf("cz", "cr", "cq")), spec("h", buf("h")), spec("hx", hx0, True)]
    if not inplace:
        specs.append(("z", N * C * HW * es, None))
    ar = arena(DEV, specs, phase, half)
    zp = view(ar, "zr", 2 * C, 0, shape, layout, es) if stacked else view(ar, "zp", C, 0, shape, layout, es)
    rp = view(ar, "zr", 2 * C, C, shape, layout, es) if stacked else view(ar, "rp", C, 0, shape, layout, es)
    ops = [zp, rp, view(ar, "ctx", 3 * C, 0, shape, layout, es), view(ar, "ctx", 3 * C, C, shape, layout, es),
           view(ar, "h", C, 0, shape, layout, es), zp if inplace else view(ar, "z", C, 0, shape, layout, es),
           view(ar, "hx", C + Cx, 0, shape, layout, es)]
    rc = _lib.lib().rc_gru_gates(*(p for p, _ in ops), _lib.long_array([s for _, t in ops for s in t]), code,
                                 N, C, HW, None)
    _lib.check(rc, "rc_gru_gates")
    torch.cuda.synchronize()
    ar.assert_guards_intact()
    ar.assert_outputs_written(["hx"] if inplace else ["hx", "z"], es)
    after = unpack(torch.from_numpy(ar.region("hx", np.uint8).copy()).view(dt), N, C + Cx, HW, layout)
    assert torch.equal(bits(after[:, C:]), bits(v["x"].to(dt))), "x channels of [r*h, x] changed"
    rh = fetch(ar, "hx", C + Cx)
    if inplace:
        zname, zk = ("zr", 2 * C) if stacked else ("zp", C)
        z = fetch(ar, zname, zk)
        if stacked:         # r_pre, the other half of the buffer z was written into
            assert torch.equal(fetch(ar, "zr", 2 * C, C).float(), v["r_pre"]), "r_pre changed"
    else:
        z = fetch(ar, "z", C)

    # ---- blend
    specs = [spec("z", buf("z")), spec("q", buf("q_pre")), spec("ctx", buf("cz", "cr", "cq")),
             spec("h", buf("h"), inplace)]
    if not inplace:
        specs.append(("out", N * C * HW * es, None))
    ar = arena(DEV, specs, phase, half)
    hv = view(ar, "h", C, 0, shape, layout, es)
    ops = [view(ar, "z", C, 0, shape, layout, es), view(ar, "q", C, 0, shape, layout, es),
           view(ar, "ctx", 3 * C, 2 * C, shape, layout, es), hv,
           hv if inplace else view(ar, "out", C, 0, shape, layout, es)]
    rc = _lib.lib().rc_gru_blend(*(p for p, _ in ops), _lib.long_array([s for _, t in ops for s in t]), code,
                                 N, C, HW, None)
    _lib.check(rc, "rc_gru_blend")
    torch.cuda.synchronize()
    ar.assert_guards_intact()
    if not inplace:
        ar.assert_outputs_written(["out"], es)
    hout = fetch(ar, "h" if inplace else "out", C)
    return z, rh, hout


@functools.lru_cache(maxsize=None)
def _result(shape, vdt, kdt, layout, stacked, inplace, phase):
    return run(values(shape, vdt), shape, kdt, layout, stacked, inplace, phase)


def result(shape, vdt, kdt, layout, stacked=True, inplace=False, phase=0):
    """``run`` on the shape's values, once per combination for the whole module."""
    return _result(shape, vdt, kdt, layout, bool(stacked), bool(inplace), int(phase))


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def same_bits(a, b, what):
    for x, y, n in zip(a, b, ("z", "r*h", "h_out")):
        assert x.dtype == y.dtype and torch.equal(bits(x), bits(y)), \
            f"{what}: {n} differs in {int((bits(x) != bits(y)).sum())} of {x.numel()} elements"


@functools.lru_cache(maxsize=None)
def references(shape):
    """(float64 evaluation, torch fp32 op sequence on the device) of the fp32 values."""
    v = values(shape, "fp32")
    n = {k: t.numpy() for k, t in v.items()}
    z64, rh64 = gru_ref.gates(n["z_pre"], n["r_pre"], n["cz"], n["cr"], n["h"])
    ref64 = (z64, rh64, gru_ref.blend(n["z"], n["q_pre"], n["cq"], n["h"]))
    d = {k: t.to(DEV) for k, t in v.items()}
    zt = torch.sigmoid(d["z_pre"] + d["cz"])
    rt = torch.sigmoid(d["r_pre"] + d["cr"])
    ht = (1 - d["z"]) * d["h"] + d["z"] * torch.tanh(d["q_pre"] + d["cq"])
    return ref64, tuple(t.cpu().numpy() for t in (zt, rt * d["h"], ht))


@pytest.mark.parametrize("phase", [0, 1])
@pytest.mark.parametrize("stacked", [True, False], ids=["stacked", "separate"])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_fp32_values(shape, layout, stacked, phase):
    got = result(shape, "fp32", "fp32", layout, stacked, False, phase)
    ref64, ref_torch = references(shape)
    for g, r64, rt, n in zip(got, ref64, ref_torch, ("z", "r*h", "h_out")):
        e64, et = norm_err(g.numpy(), r64), norm_err(g.numpy(), rt)
        print(f"{n}: norm_err {e64:.2e} vs float64, {et:.2e} vs torch fp32")
        assert np.isfinite(g.numpy()).all()
        assert e64 <= TOL and et <= TOL, (n, e64, et)
    same_bits(got, result(shape, "fp32", "fp32", layout, stacked, False, 0), "phase 1 vs phase 0")


@pytest.mark.parametrize("stacked", [True, False], ids=["stacked", "separate"])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("kdt", ["fp16", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_half_is_the_fp32_result_rounded_once(shape, kdt, layout, stacked):
    want = tuple(t.to(DT[kdt]) for t in result(shape, kdt, "fp32", layout, stacked))
    for phase in (0, 1):
        same_bits(result(shape, kdt, kdt, layout, stacked, False, phase), want, f"{kdt} phase {phase} vs fp32.to()")


@pytest.mark.parametrize("stacked", [True, False], ids=["stacked", "separate"])
@pytest.mark.parametrize("kdt", list(DT))
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_layout_classes_agree(shape, kdt, stacked):
    same_bits(result(shape, kdt, kdt, "interleaved", stacked), result(shape, kdt, kdt, "planar", stacked),
              "interleaved vs planar")
    same_bits(result(shape, kdt, kdt, "planar", stacked), result(shape, kdt, kdt, "planar", not stacked),
              "stacked vs separate")


@pytest.mark.parametrize("stacked", [True, False], ids=["stacked", "separate"])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("kdt", list(DT))
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_in_place(shape, kdt, layout, stacked):
    """z_out = z_pre and h_out = h."""
    for phase in (0, 1):
        same_bits(result(shape, kdt, kdt, layout, stacked, True, phase), result(shape, kdt, kdt, layout, stacked),
                  f"in place (phase {phase}) vs out of place")


SPECIAL = [float("inf"), float("-inf"), 1e4, -1e4, 88.9, -88.9, 0.0, -0.0, 1e-40, -1e-40, float("nan"),
           6e-8, -6e-8, 100.0, -100.0, 3e38]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("kdt", list(DT))
def test_special_values(kdt, layout):
    """pre + c at +-inf, +-1e4, +-88.9, +-100, +-0, subnormals, the largest
    finite values and NaN (c = 0, so the sum is the value; 1e-40 is an fp32
    subnormal, 6e-8 an fp16 one; each rounded to the dtype under test, where
    3e38 becomes inf in fp16): wherever |pre + c| >= 88.9 the outputs equal
    the torch fp32 op sequence's exactly (sigmoid 0 / 1, tanh +-1), NaN
    appears at the NaN input's positions only, everything else is finite and
    within the fp32 bound of torch."""
    shape = (1, 2, 1, 1, len(SPECIAL))
    N, C, Cx, H, W = shape
    dt = DT[kdt]
    g = torch.Generator().manual_seed(5)
    sp = torch.tensor(SPECIAL).to(dt).float().view(1, 1, W).expand(N, C, W).contiguous()
    v = {"z_pre": sp, "r_pre": sp.flip(-1).contiguous(), "q_pre": sp}
    for k in ("cz", "cr", "cq"):
        v[k] = torch.zeros(N, C, W)
    v["h"] = torch.tanh(torch.randn(N, C, W, generator=g)).to(dt).float()
    v["z"] = torch.rand(N, C, W, generator=g).to(dt).float()
    v["x"] = torch.randn(N, Cx, W, generator=g).to(dt).float()
    got = [t.float() for t in run(v, shape, kdt, layout)]
    d = {k: t.to(DEV) for k, t in v.items()}
    zt = torch.sigmoid(d["z_pre"] + d["cz"])
    rht = torch.sigmoid(d["r_pre"] + d["cr"]) * d["h"]
    ht = (1 - d["z"]) * d["h"] + d["z"] * torch.tanh(d["q_pre"] + d["cq"])
    want = [t.cpu().to(dt).float() for t in (zt, rht, ht)]
    args = (v["z_pre"], v["r_pre"], v["q_pre"])
    for g_, w_, a, n in zip(got, want, args, ("z", "r*h", "h_out")):
        nan = torch.isnan(a)
        assert torch.equal(torch.isnan(g_), nan), f"{n}: NaN positions"
        assert torch.equal(torch.isnan(w_), nan)
        sat = a.abs() >= 88.9
        assert torch.equal(g_[sat], w_[sat]), f"{n}: at saturation {g_[sat]} vs torch {w_[sat]}"
        assert torch.isfinite(g_[~nan]).all(), f"{n}: non-finite output"
        assert norm_err(g_[~nan].numpy(), w_[~nan].numpy()) <= (TOL if kdt == "fp32" else 2.0 ** -8), n
    z = got[0][0, 0]
    assert z[0] == 1 and z[1] == 0 and z[2] == 1 and z[3] == 0 and z[4] == 1 and z[5] == 0
    assert (z[6:10] == 0.5).all() and z[13] == 1 and z[14] == 0
