"""rc_gru_gates_backward / rc_gru_blend_backward on guarded memory (the arena
of sweep_util.py), through the raw C ABI.

The shapes, the value distributions and the layout helpers are those of
test_gru_gates_gpu.py (its docstring says which access width each shape
reaches in which layout class and dtype); z is the forward's, sigmoid(z_pre +
cz), and the incoming gradients are standard normal.  Every run carves its
operands out of one NaN-filled buffer at the arena's two sub-line phases and
checks that the guards and the inputs are bit-identical afterwards and that
every output element was written.  g_zpre / g_rpre are the halves of one
stacked (N, 2C) buffer (then r_pre is a half of the stacked pre-activations
too) or two buffers; cr / cq are thirds of one buffer.

Bounds: the fp32 results against the float64 evaluation (gru_bwd_ref.py) and
against torch fp32 autograd of the op sequence at norm_err <= 1e-5, the
project's fp32 bound (TOL of test_gru_gates_gpu.py).  Everything else is bit
equality: fp16 / bf16 against ``.to(dtype)`` of the fp32 kernel on the widened
inputs, planar against interleaved, stacked against separate, phase against
phase, in place (g_zpre over g_z, the blend's g_h over g_out) against out of
place.
"""
import functools

import numpy as np
import pytest
import torch

import gru_bwd_ref
from golden_util import norm_err
from raft_stereo_amd import _lib, gru
from sweep_util import arena
from test_gru_gates_gpu import (CODE, DEV, DT, LAYOUTS, SHAPE_IDS, SHAPES, SPECIAL, TOL, bits, pack, sentinel,
                                unpack, values, view)

pytestmark = pytest.mark.gpu
OUTS = ("g_zpre", "g_rpre", "g_h (gates)", "g_z", "g_qpre", "g_h (blend)")


@functools.lru_cache(maxsize=None)
def bwd_values(shape, vdt):
    """``values`` of test_gru_gates_gpu.py with z = sigmoid(z_pre + cz) and the
    three incoming gradients, every value representable in ``vdt``; never
    modified."""
    N, C, Cx, H, W = shape
    v = dict(values(shape, vdt))
    g = torch.Generator().manual_seed(sum(shape) + 1)
    for k in ("g_out", "g_z", "g_rh"):
        v[k] = torch.randn(N, C, H * W, generator=g)
    v["z"] = torch.sigmoid(v["z_pre"] + v["cz"])
    return {k: t.to(DT[vdt]).float() for k, t in v.items()}


def run(v, shape, kdt, layout, stacked=True, inplace=False, phase=0):
    """Both backward kernels on the values ``v`` in dtype ``kdt``; returns the
    six gradients (OUTS) as CPU tensors (N, C, HW) of that dtype."""
    N, C, Cx, H, W = shape
    HW = H * W
    dt, code = DT[kdt], CODE[kdt]
    es = 4 if kdt == "fp32" else 2
    half = es == 2
    nbytes = N * C * HW * es

    def buf(*names):
        return pack(torch.cat([v[k] for k in names], 1).to(dt), layout)

    def spec(name, t, inout=False):
        return (name, t.numel() * es, t, inout)

    def fetch(ar, name, K, c0=0):
        flat = torch.from_numpy(ar.region(name, np.uint8).copy()).view(dt)
        return unpack(flat, N, K, HW, layout)[:, c0:c0 + C].contiguous()

    def at(ar, name, K=C, c0=0):
        return view(ar, name, K, c0, shape, layout, es)

    def call(fn, name, ops):
        rc = fn(*(p for p, _ in ops), _lib.long_array([s for _, t in ops for s in t]), code, N, C, HW, None)
        _lib.check(rc, name)
        torch.cuda.synchronize()

    # ---- gates: g_z g_rh z r_pre cr h -> g_zpre g_rpre g_h
    specs = [spec("grh", buf("g_rh")), spec("z", buf("z")), spec("ctx", buf("cz", "cr", "cq")), spec("h", buf("h")),
             ("gh", nbytes, None)]
    if stacked:
        specs.append(spec("zr", buf("z_pre", "r_pre")))
        if inplace:          # g_z lies where g_zpre goes: the first half of the stacked gradient
            both = pack(torch.cat([v["g_z"].to(dt), sentinel(N * C * HW, dt).view(N, C, HW)], 1), layout)
            specs.append(spec("gzr", both, True))
        else:
            specs += [spec("gz", buf("g_z")), ("gzr", 2 * nbytes, None)]
        outs = ["gzr", "gh"]
    else:
        specs += [spec("rp", buf("r_pre")), spec("gz", buf("g_z"), inplace), ("grp", nbytes, None)]
        if not inplace:
            specs.append(("gzp", nbytes, None))
        outs = ["gz" if inplace else "gzp", "grp", "gh"]
    ar = arena(DEV, specs, phase, half)
    if stacked:
        gzp, grp, rp = at(ar, "gzr", 2 * C, 0), at(ar, "gzr", 2 * C, C), at(ar, "zr", 2 * C, C)
        gz = gzp if inplace else at(ar, "gz")
    else:
        gz = at(ar, "gz")
        gzp, grp, rp = gz if inplace else at(ar, "gzp"), at(ar, "grp"), at(ar, "rp")
    call(_lib.lib().rc_gru_gates_backward, "rc_gru_gates_backward",
         [gz, at(ar, "grh"), at(ar, "z"), rp, at(ar, "ctx", 3 * C, C), at(ar, "h"), gzp, grp, at(ar, "gh")])
    ar.assert_guards_intact()
    ar.assert_outputs_written(outs, es)
    if stacked:
        got = [fetch(ar, "gzr", 2 * C, 0), fetch(ar, "gzr", 2 * C, C)]
    else:
        got = [fetch(ar, "gz" if inplace else "gzp", C), fetch(ar, "grp", C)]
    got.append(fetch(ar, "gh", C))

    # ---- blend: g_out z q_pre cq h -> g_z g_qpre g_h
    specs = [spec("go", buf("g_out"), inplace), spec("z", buf("z")), spec("q", buf("q_pre")),
             spec("ctx", buf("cz", "cr", "cq")), spec("h", buf("h")), ("gz", nbytes, None), ("gq", nbytes, None)]
    if not inplace:
        specs.append(("gh", nbytes, None))
    ar = arena(DEV, specs, phase, half)
    go = at(ar, "go")
    call(_lib.lib().rc_gru_blend_backward, "rc_gru_blend_backward",
         [go, at(ar, "z"), at(ar, "q"), at(ar, "ctx", 3 * C, 2 * C), at(ar, "h"), at(ar, "gz"), at(ar, "gq"),
          go if inplace else at(ar, "gh")])
    ar.assert_guards_intact()
    ar.assert_outputs_written(["gz", "gq", "go" if inplace else "gh"], es)
    got += [fetch(ar, "gz", C), fetch(ar, "gq", C), fetch(ar, "go" if inplace else "gh", C)]
    return tuple(got)


@functools.lru_cache(maxsize=None)
def _result(shape, vdt, kdt, layout, stacked, inplace, phase):
    return run(bwd_values(shape, vdt), shape, kdt, layout, stacked, inplace, phase)


def result(shape, vdt, kdt, layout, stacked=True, inplace=False, phase=0):
    """``run`` on the shape's values, once per combination for the whole module."""
    return _result(shape, vdt, kdt, layout, bool(stacked), bool(inplace), int(phase))


def same_bits(a, b, what):
    for x, y, n in zip(a, b, OUTS):
        assert x.dtype == y.dtype and torch.equal(bits(x), bits(y)), \
            f"{what}: {n} differs in {int((bits(x) != bits(y)).sum())} of {x.numel()} elements"


def torch_autograd(v):
    """The six gradients by torch fp32 autograd of the op sequence on the
    device, from fp32 CPU values; z of the gates is torch's own sigmoid(z_pre
    + cz), z of the blend the given one."""
    d = {k: t.to(DEV) for k, t in v.items()}
    zp, rp, h = (d[k].clone().requires_grad_(True) for k in ("z_pre", "r_pre", "h"))
    zt = torch.sigmoid(zp + d["cz"])
    rh = torch.sigmoid(rp + d["cr"]) * h
    gates = torch.autograd.grad([zt, rh], [zp, rp, h], [d["g_z"], d["g_rh"]])
    z, qp, h = (d[k].clone().requires_grad_(True) for k in ("z", "q_pre", "h"))
    out = (1 - z) * h + z * torch.tanh(qp + d["cq"])
    blend = torch.autograd.grad([out], [z, qp, h], [d["g_out"]])
    return tuple(t.cpu() for t in gates + blend)


@functools.lru_cache(maxsize=None)
def references(shape):
    """(float64 evaluation, torch fp32 autograd on the device) of the fp32 values."""
    v = bwd_values(shape, "fp32")
    n = {k: t.numpy() for k, t in v.items()}
    ref64 = (gru_bwd_ref.gates_backward(n["g_z"], n["g_rh"], n["z"], n["r_pre"], n["cr"], n["h"]) +
             gru_bwd_ref.blend_backward(n["g_out"], n["z"], n["q_pre"], n["cq"], n["h"]))
    return ref64, tuple(t.numpy() for t in torch_autograd(v))


@pytest.mark.parametrize("phase", [0, 1])
@pytest.mark.parametrize("stacked", [True, False], ids=["stacked", "separate"])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_fp32_values(shape, layout, stacked, phase):
    got = result(shape, "fp32", "fp32", layout, stacked, False, phase)
    ref64, ref_torch = references(shape)
    for g, r64, rt, n in zip(got, ref64, ref_torch, OUTS):
        e64, et = norm_err(g.numpy(), r64), norm_err(g.numpy(), rt)
        print(f"{n}: norm_err {e64:.2e} vs float64, {et:.2e} vs torch fp32 autograd")
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
    """g_zpre over g_z and the blend's g_h over g_out."""
    for phase in (0, 1):
        same_bits(result(shape, kdt, kdt, layout, stacked, True, phase), result(shape, kdt, kdt, layout, stacked),
                  f"in place (phase {phase}) vs out of place")


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("kdt", list(DT))
def test_special_values(kdt, layout):
    """SPECIAL of test_gru_gates_gpu.py (+-inf, +-1e4, +-88.9, +-100, +-0,
    subnormals, the largest finite values, NaN; each rounded to the dtype under
    test) as r_pre, q_pre and z_pre with zero context, z from the forward
    kernel on z_pre, finite random incoming gradients.  Wherever |pre| >= 88.9
    the forward saturates, and the outputs equal torch fp32 autograd's
    exactly: g_zpre, g_rpre and g_qpre are +-0 and the gates' g_h is g_rh
    times exactly 0 or 1.  NaN appears at the NaN input's positions only;
    everything else is finite."""
    shape = (1, 2, 1, 1, len(SPECIAL))
    N, C, Cx, H, W = shape
    dt = DT[kdt]
    g = torch.Generator().manual_seed(5)
    sp = torch.tensor(SPECIAL).to(dt).float().view(1, 1, W).expand(N, C, W).contiguous()
    v = {"z_pre": sp, "r_pre": sp.flip(-1).contiguous(), "q_pre": sp}
    for k in ("cz", "cr", "cq"):
        v[k] = torch.zeros(N, C, W)
    v["h"] = torch.tanh(torch.randn(N, C, W, generator=g)).to(dt).float()
    for k in ("g_out", "g_z", "g_rh"):
        v[k] = torch.randn(N, C, W, generator=g).to(dt).float()
    low = {k: v[k].to(dt).view(N, C, 1, W).to(DEV) for k in ("z_pre", "r_pre", "cz", "cr", "h")}
    z, _ = gru.gru_gates(low["z_pre"], low["r_pre"], low["cz"], low["cr"], low["h"])
    v["z"] = z.float().cpu().view(N, C, W)
    got = [t.float() for t in run(v, shape, kdt, layout)]
    want = [t.to(dt).float() for t in torch_autograd(v)]
    zn, rn, qn = (torch.isnan(v[k]) for k in ("z_pre", "r_pre", "q_pre"))
    nans = (zn, rn, rn, qn, qn | zn, zn)
    sats = (v["z_pre"].abs() >= 88.9, v["r_pre"].abs() >= 88.9, v["r_pre"].abs() >= 88.9, None,
            v["q_pre"].abs() >= 88.9, None)
    for g_, w_, nan, sat, n in zip(got, want, nans, sats, OUTS):
        assert torch.equal(torch.isnan(g_), nan), f"{n}: NaN positions"
        assert torch.equal(torch.isnan(w_), nan), n
        assert torch.isfinite(g_[~nan]).all(), f"{n}: non-finite output"
        if sat is not None:
            assert sat.sum() >= 7 * C           # 88.9 rounds to 88.875 in fp16
            assert torch.equal(g_[sat], w_[sat]), f"{n}: at saturation {g_[sat]} vs torch {w_[sat]}"
    for k in (0, 1, 4):
        assert (got[k][sats[k]] == 0).all(), OUTS[k]
    rsat = sats[1]
    assert torch.equal(got[2][rsat], (v["g_rh"] * (v["r_pre"] > 0))[rsat]), "g_h (gates) is not g_rh times 0 or 1"
