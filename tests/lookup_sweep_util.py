"""CPU pyramids, arena placement and guarded raw C-ABI callers for the lookup
sweeps (test_lookup_sweep_gpu.py, test_lookup_sweep_host.py), on top of the
arena of sweep_util.py.

Every caller carves the pyramid levels, the coordinates and every output of
one call out of one arena, calls the entry point through ``_lib.lib()`` with
the arena's addresses and, on return, runs ``_lib.check``, then
``assert_guards_intact`` (guards and inputs bit-identical), then
``assert_outputs_written`` (no output element still the sentinel).

What the poison is: rows are padded to 16 bytes and the padding keeps the
arena's NaN pattern; with RC_SHADOW the gap between a level and its copy keeps
it too; the y channel of the coordinates is the pattern (the lookups ignore
it); levels a kernel is documented not to read are passed as NULL.  A value
taken from any of these reaches the output as a NaN the oracle does not have.

``0x7FC1`` is a NaN as fp16 as well as bf16, so ``Arena(bf16=True)`` serves
fp16 pyramids and fp16 outputs.
"""
import numpy as np
import torch

import sweep_util as su
from oracle import coracle
from raft_stereo_amd import _lib

KINDS = ("f32", "bf16", "f16")
ES = {"f32": 4, "bf16": 2, "f16": 2}
CODE = {"f32": _lib.RC_F32, "bf16": _lib.RC_BF16, "f16": _lib.RC_F16}
POOL = {"f32": coracle.corr_pool, "bf16": su.bf16_pool_np, "f16": su.f16_pool_np}
SENT_PAIR = su.SENT16 << 16 | su.SENT16
OUT_DT = {_lib.RC_OUT_F16: torch.float16, _lib.RC_OUT_BF16: torch.bfloat16}
OUT_HALF = _lib.RC_OUT_F16 | _lib.RC_OUT_BF16


# ------------------------------------------------------------ CPU pyramid

def round_kind(a, kind):
    """fp32 values rounded to the element type (nearest even), widened again."""
    a = np.ascontiguousarray(a, np.float32)
    if kind == "bf16":
        return torch.from_numpy(a).bfloat16().float().numpy()
    if kind == "f16":
        return a.astype(np.float16).astype(np.float32)
    return a


def cpu_pyramid(P, W2, L, kind, seed):
    """L levels (P, W2 >> l) as fp32 arrays, made without the project's build:
    level 0 random, rounded to the element type; each higher level the pool of
    the level below as stored."""
    g = torch.Generator().manual_seed(seed)
    pyr = [round_kind(torch.randn(P, W2, generator=g).numpy(), kind)]
    for _ in range(1, L):
        pyr.append(POOL[kind](pyr[-1]))
    return pyr


def to_bits(level, kind):
    """The stored bits of a level given as fp32 values of its element type."""
    level = np.ascontiguousarray(level, np.float32)
    if kind == "f32":
        return level.view(np.uint32)
    if kind == "bf16":
        assert not (level.view(np.uint32) & 0xFFFF).any(), "not bf16 values"
        return (level.view(np.uint32) >> 16).astype(np.uint16)
    return level.astype(np.float16).view(np.uint16)


def sent32(bf):
    return SENT_PAIR if bf else su.SENT32


# -------------------------------------------------------------- placement

def level_image(level, kind, bf, shadow=False):
    """One level as it lies in the arena: rows padded to 16 bytes, the padding
    the sentinel; with ``shadow`` the copy at RC_SHADOW_OFFSET after it and
    the gap the sentinel.  Returns (int32 tensor, row stride in elements)."""
    P, W = level.shape
    es = ES[kind]
    ld = su.level_ld(W, torch.bfloat16 if es == 2 else torch.float32, True)
    n = P * ld * es
    off = _lib.shadow_offset(P, ld, es)
    img = np.full(((off + n) if shadow else n) // 4, sent32(bf), np.uint32)
    bits = to_bits(level, kind)
    v = img.view(bits.dtype)
    v[:P * ld].reshape(P, ld)[:, :W] = bits
    if shadow:
        v[off // es:off // es + P * ld].reshape(P, ld)[:, :W] = bits
    return torch.from_numpy(img.view(np.int32)), ld


def coords_image(x, bf, y=None):
    """(B, 2, H, W1) coordinates as int32 bits: x as given, the y channel the
    sentinel NaN (ignored by the lookups) unless given."""
    B, H, W1 = x.shape
    img = np.full((B, 2, H, W1), sent32(bf), np.uint32)
    img[:, 0] = np.ascontiguousarray(x, np.float32).view(np.uint32)
    if y is not None:
        img[:, 1] = np.ascontiguousarray(y, np.float32).view(np.uint32)
    return torch.from_numpy(img.view(np.int32))


def f32_spec(name, a):
    t = torch.from_numpy(np.ascontiguousarray(a, np.float32))
    return (name, t.numel() * 4, t)


class Levels:
    """The arena regions and C-ABI arrays of one pyramid.

    ``rows(pyr, kind, stored, shadow, bf)``: a CPU pyramid in rows; ``stored``
    the levels given a buffer (the others NULL), ``shadow`` the stored levels
    that carry a copy ("all": RC_SHADOW, every stored level).
    The constructor takes regions prepared elsewhere (records,
    disparity-major levels from a guarded build)."""

    def __init__(self, specs, names, widths, lds, dtype_flags):
        self.specs, self.names, self.widths, self.lds, self.dtype_flags = specs, names, widths, lds, dtype_flags

    @classmethod
    def rows(cls, pyr, kind, stored=None, shadow=(), bf=False):
        L = len(pyr)
        stored = tuple(range(L)) if stored is None else tuple(stored)
        flags = CODE[kind]
        if shadow == "all":
            shadow, flags = stored, flags | _lib.RC_SHADOW
        else:
            for l in shadow:
                assert l in stored
                flags |= _lib.shadow_level(l)
        specs, names, lds = [], [], []
        for l in range(L):
            if l not in stored:
                names.append(None)
                lds.append(pyr[l].shape[1])
                continue
            t, ld = level_image(pyr[l], kind, bf, l in shadow)
            specs.append((f"l{l}", t.numel() * 4, t))
            names.append(f"l{l}")
            lds.append(ld)
        return cls(specs, names, [p.shape[1] for p in pyr], lds, flags)

    def args(self, ar):
        """(pyr, widths, pyr_ld) of the C ABI for arena ``ar``."""
        return (_lib.ptr_array([None if n is None else ar.ptr(n) for n in self.names]),
                _lib.int_array(self.widths), None if self.lds is None else _lib.long_array(self.lds))


def finish(ar, rc, what, outs):
    """The checks every guarded caller ends with.  outs: {output region:
    element size}."""
    _lib.check(rc, what)
    ar.assert_guards_intact()
    for name, es in outs.items():
        ar.assert_outputs_written([name], es)


def read_out(ar, name, shape, out_dt, cl):
    """An output region as (B, C, H, W1): fp32 numpy array, or a torch tensor
    of the 16-bit type."""
    B, C, H, W1 = shape
    lay = (B, H, W1, C) if cl else shape
    if out_dt is None:
        a = ar.region(name, np.float32).reshape(lay).copy()
        return a.transpose(0, 3, 1, 2) if cl else a
    t = torch.from_numpy(ar.region(name, np.int16).copy()).view(out_dt).view(lay)
    return t.permute(0, 3, 1, 2) if cl else t


def first_bad(rcs):
    return next((rc for rc in rcs if rc != _lib.RC_OK), _lib.RC_OK)


# ------------------------------------------------------------ coordinates

def smooth_field(B, H, W1, W2):
    """One smooth in-range field: x runs over the row's width with a slow
    wobble, shifted per image row and batch."""
    w = np.arange(W1, dtype=np.float32)[None, None, :]
    h = np.arange(H, dtype=np.float32)[None, :, None]
    b = np.arange(B, dtype=np.float32)[:, None, None]
    x = w * np.float32((W2 - 1) / max(W1 - 1, 1)) - np.float32(2.75) * np.sin(np.float32(0.21) * w + h) \
        - np.float32(0.5) * h - np.float32(1.25) * b
    return np.ascontiguousarray(x, np.float32)


def coord_sets(B, H, W1, W2, seed):
    """The x arrays (B, H, W1) of one case: test_corr_gpu.special_coords (NaN,
    +-inf, +-1e30, +-0, subnormals, far out of range, random integers and
    fractions); the integer sweep -40 .. W2 + 40 with both fp32 neighbours, in
    as many arrays as it needs (the last filled up from the smooth field); one
    smooth field.  {"special": [x], "sweep": [x, ..], "smooth": [x]}"""
    from test_corr_gpu import special_coords
    g = torch.Generator().manual_seed(seed)
    sp = special_coords(B, H, W1, W2, g)[:, 0].contiguous().numpy()
    sm = smooth_field(B, H, W1, W2)
    P = B * H * W1
    sw = su.integer_sweep(W2)
    sw = np.concatenate([sw, sm.reshape(-1)[:-len(sw) % P]])
    return {"special": [sp], "sweep": [c.reshape(B, H, W1).copy() for c in sw.reshape(-1, P)], "smooth": [sm]}


def all_sets(cs):
    return cs["special"] + cs["sweep"] + cs["smooth"]


def finite_sets(cs):
    return cs["sweep"] + cs["smooth"]


def packed_coords(B, H, W1, W2, seed):
    """One (B, H, W1) array holding all three coordinate sets of coord_sets(1,
    1, 70, W2), repeated to fill it (the large-P cases)."""
    vals = np.concatenate([c.reshape(-1) for c in all_sets(coord_sets(1, 1, 70, W2, seed))])
    n = B * H * W1
    return np.resize(vals, n).reshape(B, H, W1).astype(np.float32)


def as_coords(x):
    """(B, 2, H, W1) for the oracle: x, and y = 0."""
    B, H, W1 = x.shape
    c = np.zeros((B, 2, H, W1), np.float32)
    c[:, 0] = x
    return c


# ------------------------------------------------------- guarded forwards

def guarded_lookup(dev, entry, lv, L, r, xs, flags=0, phase=0, bf=False):
    """rc_corr_lookup / rc_corr_lookup_chain (``entry``) on arena memory, once
    per coordinate array of ``xs`` (each (B, H, W1) fp32, with a coords and an
    output region of its own; the levels are shared).  lv: Levels made with
    the same ``bf``; flags: RC_OUT_* / RC_LAYOUT_* bits.  Returns the outputs
    as read_out gives them."""
    B, H, W1 = xs[0].shape
    C = L * (2 * r + 1)
    out_dt = OUT_DT.get(flags & OUT_HALF)
    es = 4 if out_dt is None else 2
    assert bf or (es == 4 and lv.dtype_flags & 0xFF == _lib.RC_F32)
    specs = list(lv.specs)
    for k, x in enumerate(xs):
        c = coords_image(x, bf)
        specs += [(f"coords{k}", c.numel() * 4, c), (f"out{k}", B * C * H * W1 * es, None)]
    ar = su.arena(dev, specs, phase, bf)
    pyr, widths, lds = lv.args(ar)
    fn = getattr(_lib.lib(), entry)
    rcs = [fn(pyr, widths, lds, lv.dtype_flags | flags, L, r, ar.ptr(f"coords{k}"), 2 * H * W1, B, H, W1,
              ar.ptr(f"out{k}"), None) for k in range(len(xs))]
    finish(ar, first_bad(rcs), entry, {f"out{k}": es for k in range(len(xs))})
    cl = bool(flags & _lib.RC_OUT_CHANNELS_LAST)
    return [read_out(ar, f"out{k}", (B, C, H, W1), out_dt, cl) for k in range(len(xs))]


def coords_grid(B, H, W1):
    """coords0 of the reference (model.py:329-332): x = w, y = h."""
    ys, xs = torch.meshgrid(torch.arange(H).float(), torch.arange(W1).float(), indexing="ij")
    return torch.stack([xs, ys], 0)[None].repeat(B, 1, 1, 1)


def guarded_step(dev, lv, L, r, coords1, delta_x, alias, flags=0, phase=0, bf=False):
    """rc_corr_lookup_step with chain != 0 on arena memory.  coords1: (B, 2,
    H, W1) fp32 tensor, y finite; delta_x: (B, H, W1) array or None -- delta's
    y channel is the sentinel NaN; alias: coords1_out is coords1 (an in/out
    region).  Returns (out, coords1_out, flow_out)."""
    B, _, H, W1 = coords1.shape
    C = L * (2 * r + 1)
    out_dt = OUT_DT.get(flags & OUT_HALF)
    es = 4 if out_dt is None else 2
    n = B * 2 * H * W1 * 4
    c1 = coords1.contiguous()
    specs = lv.specs + [("coords1", n, c1, True) if alias else ("coords1", n, c1)]
    if delta_x is not None:
        specs.append(("delta", n, coords_image(delta_x, bf)))
    if not alias:
        specs.append(("coords1_out", n, None))
    specs += [("flow", n, None), ("out", B * C * H * W1 * es, None)]
    ar = su.arena(dev, specs, phase, bf)
    pyr, widths, lds = lv.args(ar)
    cout = "coords1" if alias else "coords1_out"
    rc = _lib.lib().rc_corr_lookup_step(pyr, widths, lds, lv.dtype_flags | flags, L, r, 1, ar.ptr("coords1"),
                                        ar.ptr("delta") if delta_x is not None else None, ar.ptr(cout),
                                        ar.ptr("flow"), B, H, W1, ar.ptr("out"), None)
    finish(ar, rc, "rc_corr_lookup_step", {cout: 4, "flow": 4, "out": es})
    shape = (B, 2, H, W1)
    return (read_out(ar, "out", (B, C, H, W1), out_dt, bool(flags & _lib.RC_OUT_CHANNELS_LAST)),
            ar.region(cout, np.float32).reshape(shape).copy(), ar.region("flow", np.float32).reshape(shape).copy())


def guarded_conv(dev, entry, lv, L, r, xs, weight, bias, relu, flags=0, phase=0, bf=False):
    """rc_corr_lookup_conv / rc_corr_lookup_chain_conv on arena memory, once
    per coordinate array of ``xs``.  weight (cout, cin), bias (cout,) or None:
    fp32 arrays.  Returns the (B, cout, H, W1) outputs (fp32 arrays, or 16-bit
    tensors)."""
    B, H, W1 = xs[0].shape
    cout = weight.shape[0]
    out_dt = OUT_DT.get(flags & OUT_HALF)
    es = 4 if out_dt is None else 2
    specs = lv.specs + [f32_spec("weight", weight)]
    if bias is not None:
        specs.append(f32_spec("bias", bias))
    for k, x in enumerate(xs):
        c = coords_image(x, bf)
        specs += [(f"coords{k}", c.numel() * 4, c), (f"out{k}", B * cout * H * W1 * es, None)]
    ar = su.arena(dev, specs, phase, bf)
    pyr, widths, lds = lv.args(ar)
    fn = getattr(_lib.lib(), entry)
    rcs = [fn(pyr, widths, lds, lv.dtype_flags | flags, L, r, ar.ptr(f"coords{k}"), 2 * H * W1, B, H, W1,
              ar.ptr("weight"), ar.ptr("bias") if bias is not None else None, cout, int(relu), ar.ptr(f"out{k}"),
              None) for k in range(len(xs))]
    finish(ar, first_bad(rcs), entry, {f"out{k}": es for k in range(len(xs))})
    return [read_out(ar, f"out{k}", (B, cout, H, W1), out_dt, False) for k in range(len(xs))]


# ------------------------------------------------------ guarded backwards

def grad_image(init, W, P, shadow=False):
    """A gradient level in the arena: (P, grad_ld(W)) fp32 rows holding
    ``init`` (P, grad_ld(W)); with ``shadow`` a zeroed copy at
    RC_SHADOW_OFFSET and the sentinel in the gap."""
    ld = su.grad_ld(W)
    n = P * ld * 4
    if not shadow:
        return torch.from_numpy(np.ascontiguousarray(init, np.float32).view(np.int32).reshape(-1))
    off = _lib.shadow_offset(P, ld, 4)
    img = np.full((off + n) // 4, su.SENT32, np.uint32)
    img[:P * ld] = np.ascontiguousarray(init, np.float32).view(np.uint32).reshape(-1)
    img[off // 4:] = 0
    return torch.from_numpy(img.view(np.int32))


def guarded_lookup_backward(dev, widths, present, L, r, xs, gouts, inits, shadow=(), phase=0, chain=False):
    """rc_corr_lookup_backward on arena memory, once per (x, grad_out, init)
    of the lists, each call with gradient buffers of its own -- or, with
    ``chain``, every call into the first call's buffers.  present: the levels
    given a buffer (pair layout: (0,) or (0, 2)); inits[k]: {level: (P,
    grad_ld(W)) fp32}, the buffers' contents before the call (in/out regions:
    the kernel accumulates); shadow: levels with a zeroed copy, the gap before
    it the sentinel.  Returns per call {level: (P, grad_ld(W)) fp64 after the
    call, the copy added in}, the row padding included."""
    B, H, W1 = xs[0].shape
    P = B * H * W1
    specs = []
    for k, (x, go) in enumerate(zip(xs, gouts)):
        c = coords_image(x, False)
        specs += [(f"coords{k}", c.numel() * 4, c), f32_spec(f"gout{k}", go)]
        if chain and k:
            continue
        for l in present:
            t = grad_image(inits[k][l], widths[l], P, l in shadow)
            specs.append((f"g{l}_{k}", t.numel() * 4, t, True))
    ar = su.arena(dev, specs, phase)
    lv = L
    for l in shadow:
        lv |= _lib.shadow_level(l)
    wid, lds = _lib.int_array(widths), _lib.long_array([su.grad_ld(w) for w in widths])
    rcs = []
    for k in range(len(xs)):
        kb = 0 if chain else k
        rcs.append(_lib.lib().rc_corr_lookup_backward(
            _lib.ptr_array([ar.ptr(f"g{l}_{kb}") if l in present else None for l in range(L)]), wid, lds, lv, r,
            ar.ptr(f"coords{k}"), 2 * H * W1, B, H, W1, ar.ptr(f"gout{k}"), None))
    finish(ar, first_bad(rcs), "rc_corr_lookup_backward", {})
    outs = []
    for k in range(1 if chain else len(xs)):
        out = {}
        for l in present:
            ld = su.grad_ld(widths[l])
            raw = ar.region(f"g{l}_{k}", np.uint32)
            got = raw[:P * ld].view(np.float32).reshape(P, ld).astype(np.float64)
            if l in shadow:
                off = _lib.shadow_offset(P, ld, 4) // 4
                assert (raw[P * ld:off] == su.SENT32).all(), f"level {l}: the gap before the copy changed"
                got = got + raw[off:].view(np.float32).reshape(P, ld)
            out[l] = got
        outs.append(out)
    return outs


def guarded_lookup_backward_calls(dev, widths, L, r, xs, gouts, init=None, phase=0):
    """rc_corr_lookup_backward_calls on the pair layout on arena memory.  xs,
    gouts: per call (B, H, W1) and (B, C, H, W1) fp32.  init None: overwrite
    mode into sentinel-filled output regions (every element must be written);
    else accumulate into in/out regions holding init[level].  Returns
    {level: (P, grad_ld(W))}."""
    B, H, W1 = xs[0].shape
    P = B * H * W1
    present = tuple(range(0, L, 2))
    specs = []
    for k, (x, go) in enumerate(zip(xs, gouts)):
        c = coords_image(x, False)
        specs += [(f"coords{k}", c.numel() * 4, c), f32_spec(f"gout{k}", go)]
    for l in present:
        n = P * su.grad_ld(widths[l]) * 4
        specs.append((f"g{l}", n, None) if init is None else (f"g{l}", n, grad_image(init[l], widths[l], P), True))
    ar = su.arena(dev, specs, phase)
    n = len(xs)
    rc = _lib.lib().rc_corr_lookup_backward_calls(
        _lib.ptr_array([ar.ptr(f"g{l}") if l in present else None for l in range(L)]), _lib.int_array(widths),
        _lib.long_array([su.grad_ld(w) for w in widths]), L | (_lib.RC_GRAD_OVERWRITE if init is None else 0), r, n,
        _lib.ptr_array([ar.ptr(f"coords{k}") for k in range(n)]), _lib.long_array([2 * H * W1] * n), B, H, W1,
        _lib.ptr_array([ar.ptr(f"gout{k}") for k in range(n)]), None)
    finish(ar, rc, "rc_corr_lookup_backward_calls", {f"g{l}": 4 for l in present} if init is None else {})
    return {l: ar.region(f"g{l}", np.float32).reshape(P, su.grad_ld(widths[l])).copy() for l in present}


CONV_BWD_OUTS = ("grad_corr", "grad_weight", "grad_bias")


def guarded_conv_backward(dev, entry, lv, L, r, x, weight, bias, relu, gout, want=CONV_BWD_OUTS, phase=0):
    """rc_corr_lookup_conv_backward / rc_corr_lookup_chain_conv_backward on
    arena memory; ``want``: the outputs asked for (the others NULL).  The
    workspace is an output region of exactly RC_LOOKUP_CONV_BWD_WS floats,
    given only when grad_weight or grad_bias is asked for.  Returns {name:
    fp32 array}."""
    B, H, W1 = x.shape
    P = B * H * W1
    cout, cin = weight.shape
    bf = lv.dtype_flags & 0xFF != _lib.RC_F32
    c = coords_image(x, bf)
    specs = lv.specs + [("coords", c.numel() * 4, c), f32_spec("weight", weight), f32_spec("gout", gout)]
    if bias is not None:
        specs.append(f32_spec("bias", bias))
    shapes = {"grad_corr": (B, cin, H, W1), "grad_weight": (cout, cin), "grad_bias": (cout,)}
    for name in want:
        specs.append((name, int(np.prod(shapes[name])) * 4, None))
    sums = "grad_weight" in want or "grad_bias" in want
    if sums:
        specs.append(("ws", _lib.lookup_conv_bwd_ws(P, cout, cin) * 4, None))
    ar = su.arena(dev, specs, phase, bf)
    pyr, widths, lds = lv.args(ar)
    rc = getattr(_lib.lib(), entry)(pyr, widths, lds, lv.dtype_flags, L, r, ar.ptr("coords"), 2 * H * W1, B, H, W1,
                                    ar.ptr("weight"), ar.ptr("bias") if bias is not None else None, cout,
                                    int(relu), ar.ptr("gout"), *[ar.ptr(n) if n in want else None
                                                                for n in CONV_BWD_OUTS],
                                    ar.ptr("ws") if sums else None, None)
    finish(ar, rc, entry, {n: 4 for n in want})
    return {n: ar.region(n, np.float32).reshape(shapes[n]).copy() for n in want}


# --------------------------------------------------------------- geometry
# Restatements of the lookup dispatch, for the docstring table of
# test_lookup_sweep_gpu.py and the assertions of test_lookup_sweep_host.py.

LEVELPAR_P = 64 * 1024            # csrc/lookup.hip, kLevelParP
SMALL_P = 256 * 256 * 2           # csrc/lookup.hip, kSmallP


def level_kernel(P, L, kind):
    """csrc/lookup.hip, launch_r (fp32 / bf16 levels) and csrc/lookup_f16pyr.hip
    (fp16 levels): the kernel rc_corr_lookup runs."""
    if kind == "f16":
        return "f16pyr_level"
    if P < LEVELPAR_P and L <= 4:
        return "levelpar"
    if P < SMALL_P and L in (3, 4):
        return "unrolled64"
    return "runtime_loop"


def chain_kernel(L, stored):
    """capi.cpp, chain_kind: the kernel rc_corr_lookup_chain runs."""
    if L == 2 or (L == 4 and 2 in stored):
        return "pair"
    if L in (3, 4) and 1 in stored:
        return "level1_chain"
    return None


def cl_tail(P, C, es):
    """csrc/lookup_pair.h, the channels-last tile: valid elements of the last
    (partial) wave's run modulo the elements of a 16-B vector; non-zero: the
    last vector goes out element by element."""
    return (P % 64) * C % (16 // es)


# ------------------------------------------------------------ sweep lists
# Shared by the GPU sweeps and the host-side coverage assertions.

SHAPES = [(1, 1, 37), (2, 1, 37), (1, 2, 70), (2, 2, 70)]      # (B, H, W1): P = 37, 74, 140, 280


def shape_for(i):
    return SHAPES[i % 4]


PAIR4_W2 = list(range(16, 144))                     # part a, L = 4
PAIR2_W2 = list(range(4, 68))                       # part a, L = 2
PAIR_BANDS = {4: su.bands(PAIR4_W2, 16), 2: su.bands(PAIR2_W2, 16)}
PAIR_MID_R = {4: {2: [16, 23, 37, 64, 77, 100, 129, 143], 3: [17, 30, 45, 63, 82, 111, 128, 142]},
              2: {2: [4, 7, 13, 22, 33, 48, 61, 67], 3: [5, 6, 15, 24, 35, 50, 64, 66]}}


def pair_kinds(W2):
    """Part a: fp32 at every width; bf16 and fp16 at every second one, the
    parity flipping every 32 widths."""
    return ["f32", "bf16" if (W2 + W2 // 32) % 2 == 0 else "f16"]


def pair_radii(W2, L):
    return [1, 4] + [r for r in (2, 3) if W2 in PAIR_MID_R[L][r]]


PAIR_FLAG_NAMES = ["none", "shadow", "shadow2", "cl", "f16", "bf16", "cl_f16", "cl_bf16"]
CL_TAIL_W1 = (65, 37)                               # B = H = 1: P % 64 = 1 and 37
CL_TAIL_W2 = {2: 21, 4: 77}
CHAIN_W2 = {4: list(range(16, 80)), 3: list(range(8, 72))}      # part b


def level_w2(L):
    """Part c: about 16 widths between 2^L and 2^L + 70, odd and even."""
    lo = 1 << L
    return sorted({lo, lo + 1, lo + 2, lo + 3, lo + 5, lo + 8, lo + 13, lo + 16, lo + 21, lo + 27, lo + 32,
                   lo + 39, lo + 47, lo + 56, lo + 63, lo + 70})


LARGE_P = [(1, 937, 70), (1, 1873, 70)]             # part c: P = 65,590 and 131,110 at W2 = 16
# part d: 16 of su.DISP_SHAPES (W1, W2), W2 >= 16 (four levels of width >= 2)
DISP_LOOKUP = ([(w, p) for w in (20, 52, 100, 132) for p in (16, 100)] +
               [(p, w) for w in (20, 36, 68, 124) for p in (44, 132)])
REC_LOOKUP_W2 = [65, 97, 128, 161, 200, 257, 311, 320]           # REC_W2's extremes + six interior
STEP_W2 = [16, 21, 37, 64, 77, 100, 129, 143]
CONV_W2 = [16, 17, 23, 37, 50, 64, 77, 96, 101, 129, 130, 143]
BWD_W2 = [16, 17, 18, 19, 24, 37, 50, 63, 64, 77, 96, 101, 110, 128, 131, 143]
CALLS_W2 = [16, 21, 37, 64, 77, 98, 128, 143]
CONV_BWD_P = [(1, 1, 37), (1, 1, 256), (1, 1, 257), (1, 3, 171)]  # P = 37, 256, 257, 513
