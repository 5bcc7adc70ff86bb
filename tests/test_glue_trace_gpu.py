"""C-ABI call trace of the Python glue in ``raft_stereo_amd/corr.py``.

Every way of reaching the kernels goes through ``corr.py``; this test pins
what the glue hands to libraftcorr for each combination of constructor
options and each method, so the glue can be restructured without moving
anything at the C-ABI boundary.  A recording proxy is installed in
``_lib._active`` (the hook the dev-library switch uses); it forwards every
``rc_*`` call to the real library and records the entry point and its
arguments: ints verbatim, pointers (the stream included) as null / non-null,
ctypes arrays element by element.  Per scenario the trace also holds dtype,
shape and strides of every tensor returned (and the block's attributes), or
the class and message of the exception raised.  The traces are compared with
``tests/golden/glue_trace.json``; ``RAFT_GLUE_TRACE_REGEN=1`` rewrites that
file instead (any other value: the path to write to).

The trace sees the shape of a call, not its data: a pointer is recorded only
as null or non-null, so handing the kernel the wrong level's pointer or a
stale copy leaves the trace unchanged -- the numeric tests of the lookups, the
fused conv and the backwards catch that, this one does not.

Shapes are the smallest that reach each branch (a few thousand pixels at the
most), not workload shapes.  Reference: model.py:283-326."""
import ctypes
import json
import os

import pytest
import torch

from raft_stereo_amd import CorrBlock1D, _lib, coords_grid
from raft_stereo_amd import corr as rcorr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "glue_trace.json")
REGEN = os.environ.get("RAFT_GLUE_TRACE_REGEN", "")

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DEFAULT = (2, 32, 3, 40, 40)        # B, D, H, W1, W2
PADDED = (2, 32, 3, 40, 37)         # W2 >> l no 16-byte multiple: row-padded levels
RECORDS = (1, 256, 2, 72, 72)       # what records_supported asks for
ONE = (1, 32, 3, 40, 40)            # B = 1: cbs takes its other branch


# ------------------------------------------------------------ the recorder

def _enc(ctype, v):
    if ctype is ctypes.c_void_p:
        return "ptr" if v else "null"
    if ctype in (ctypes.c_int, ctypes.c_long):
        return int(v)
    if v is None:
        return "null"
    if ctype._type_ is ctypes.c_void_p:
        return ["ptr" if e else "null" for e in v]
    return [int(e) for e in v]


class _Recorder:
    """Stands in for the CDLL: forwards everything, records the rc_* calls."""

    def __init__(self, real):
        self._real = real
        self.calls = []

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if name not in _lib.SIGNATURES or name in ("rc_abi_version", "rc_last_error"):
            return fn
        argtypes = _lib.SIGNATURES[name][1]

        def call(*args):
            assert len(args) == len(argtypes), name
            self.calls.append([name] + [_enc(t, a) for t, a in zip(argtypes, args)])
            return fn(*args)
        return call


def _desc(o):
    if isinstance(o, torch.Tensor):
        return {"dtype": str(o.dtype), "shape": list(o.shape), "strides": list(o.stride())}
    if isinstance(o, (list, tuple)):
        return [_desc(x) for x in o]
    if isinstance(o, dict):
        return {str(k): _desc(v) for k, v in o.items()}
    if isinstance(o, (set, frozenset)):
        return sorted(o)
    if isinstance(o, torch.dtype):
        return str(o)
    return o


def _block(b):
    s = b._state
    return {"layout": b.layout, "num_levels": b.num_levels, "radius": b.radius, "out_dtype": b.out_dtype,
            "pyramid_dtype": b.pyramid_dtype, "channels_last": b.channels_last, "_chain": b._chain,
            "_shadow": b._shadow, "levels_stored": b.levels_stored, "_levels": b._levels,
            "_records": b._records, "_sheared": b._sheared, "_token": b._token,
            "_state": None if s is None else {
                "P": s.P, "widths": s.widths, "pair": s.pair, "deferred": s.deferred,
                "grad_shadow": s.grad_shadow, "exact_f32": s.exact_f32, "num_levels": s.num_levels,
                "radius": s.radius}}


# ----------------------------------------------------------------- inputs

def fmaps(shape=DEFAULT, dtype=F32, grad=False):
    B, D, H, W1, W2 = shape
    g = torch.Generator().manual_seed(7)
    f1 = torch.randn(B, D, H, W1, generator=g).to(DEV, dtype).requires_grad_(grad)
    f2 = torch.randn(B, D, H, W2, generator=g).to(DEV, dtype).requires_grad_(grad)
    return f1, f2


def coords(shape=DEFAULT, seed=3):
    B, _, H, W1, _ = shape
    g = torch.Generator().manual_seed(seed)
    c = coords_grid(B, H, W1)
    c[:, 0] -= torch.rand(B, H, W1, generator=g) * 8
    return c.to(DEV)


def convc1(blk, cout=8, bias=True, grad=False):
    cin = blk.num_levels * (2 * blk.radius + 1)
    g = torch.Generator().manual_seed(11)
    w = torch.randn(cout, cin, 1, 1, generator=g).to(DEV).requires_grad_(grad)
    b = torch.randn(cout, generator=g).to(DEV).requires_grad_(grad) if bias else None
    return w, b


def block(shape=DEFAULT, dtype=F32, grad=False, **kw):
    f1, f2 = fmaps(shape, dtype, grad)
    if grad:
        return CorrBlock1D(f1, f2, **kw), f1, f2
    with torch.no_grad():
        return CorrBlock1D(f1, f2, **kw)


# -------------------------------------------------------------- scenarios

SCENARIOS = {}


def scenario(name, *args, **kw):
    def deco(fn):
        assert name not in SCENARIOS, name
        SCENARIOS[name] = lambda: fn(*args, **kw)
        return fn
    return deco


def _call(shape=DEFAULT, dtype=F32, **kw):
    """Construct, describe the block, look up once."""
    blk = block(shape, dtype, **kw)
    with torch.no_grad():
        return _block(blk), blk(coords(shape))


CTORS = {
    "L2": dict(num_levels=2), "L3": dict(num_levels=3), "L4": dict(), "L5": dict(num_levels=5),
    "L4_r5": dict(radius=5), "L2_r5": dict(num_levels=2, radius=5),
    "low_latency": dict(low_latency=True), "eager": dict(lazy_levels=False),
    "eager_L3": dict(num_levels=3, lazy_levels=False),
    "shadow_true": dict(shadow=True), "shadow_false": dict(shadow=False), "shadow_0": dict(shadow=(0,)),
    "L2_shadow_true": dict(num_levels=2, shadow=True),
    "channels_last": dict(channels_last=True), "L3_channels_last": dict(num_levels=3, channels_last=True),
    "low_latency_channels_last": dict(low_latency=True, channels_last=True),
    "out_f16": dict(out_dtype=F16), "out_bf16": dict(out_dtype=BF16), "out_f32": dict(out_dtype=F32),
    "L3_out_f16": dict(num_levels=3, out_dtype=F16),
    "L3_channels_last_out_bf16": dict(num_levels=3, channels_last=True, out_dtype=BF16),
    "low_latency_out_f16": dict(low_latency=True, out_dtype=F16),
    "channels_last_out_f16": dict(channels_last=True, out_dtype=F16),
    "pyr_bf16": dict(pyramid_dtype=BF16), "pyr_f16": dict(pyramid_dtype=F16),
    "pyr_bf16_L3": dict(pyramid_dtype=BF16, num_levels=3),
    "pyr_f16_L2_out_f16": dict(pyramid_dtype=F16, num_levels=2, out_dtype=F16),
    "exact_f32": dict(exact_f32=True),
    "disparity_L2": dict(layout="disparity", num_levels=2), "disparity_L4": dict(layout="disparity"),
    "disparity_out_f16": dict(layout="disparity", out_dtype=F16),
    "auto": dict(layout="auto"),
}
for _n, _kw in CTORS.items():
    scenario("call/" + _n, **_kw)(_call)
for _n, _kw in (("L4", {}), ("L2", dict(num_levels=2)), ("L3", dict(num_levels=3)),
                ("low_latency", dict(low_latency=True)), ("shadow_true", dict(shadow=True)),
                ("pyr_bf16", dict(pyramid_dtype=BF16)), ("channels_last", dict(channels_last=True))):
    scenario("call/padded_" + _n, PADDED, **_kw)(_call)
for _n, _kw in (("L4", {}), ("L3", dict(num_levels=3)), ("low_latency", dict(low_latency=True)),
                ("disparity", dict(layout="disparity"))):
    scenario("call/B1_" + _n, ONE, **_kw)(_call)
for _n, _kw in (("L4", {}), ("L2", dict(num_levels=2)), ("auto", dict(layout="auto"))):
    scenario("call/bf16_fmaps_" + _n, DEFAULT, BF16, **_kw)(_call)
    scenario("call/f16_fmaps_" + _n, DEFAULT, F16, **_kw)(_call)
scenario("call/f16_fmaps_f16_pyramid", DEFAULT, F16, pyramid_dtype=F16)(_call)
for _n, _kw in (("records", dict(layout="records")), ("records_r2", dict(layout="records", radius=2)),
                ("records_channels_last_out_f16", dict(layout="records", channels_last=True, out_dtype=F16)),
                ("records_out_bf16", dict(layout="records", out_dtype=BF16)),
                ("records_auto", dict(layout="auto")), ("records_shape_rows", dict())):
    scenario("call/" + _n, RECORDS, BF16, **_kw)(_call)
scenario("call/records_f32_fmaps", RECORDS, F32, layout="records", pyramid_dtype=BF16)(_call)
scenario("call/empty_B0", (0, 32, 3, 40, 40))(_call)
scenario("call/empty_H0", (2, 32, 0, 40, 40))(_call)
scenario("call/empty_H0_L3_out_f16", (2, 32, 0, 40, 40), num_levels=3, out_dtype=F16)(_call)
scenario("call/empty_B0_low_latency", (0, 32, 3, 40, 40), low_latency=True)(_call)
scenario("call/empty_B0_records", (0, 256, 2, 72, 72), BF16, layout="records")(_call)
scenario("call/empty_H0_disparity", (1, 32, 0, 40, 40), layout="disparity")(_call)
scenario("call/empty_W1_0", (2, 32, 3, 0, 40))(_call)
scenario("call/empty_W1_0_disparity", (2, 32, 3, 0, 40), layout="disparity")(_call)
scenario("call/empty_W1_0_records", (1, 256, 2, 0, 72), BF16, layout="records")(_call)


@scenario("call/mixed_fmaps")
def _mixed():
    f1, f2 = fmaps()
    with torch.no_grad():
        blk = CorrBlock1D(f1.bfloat16(), f2)
        return _block(blk), blk(coords())


@scenario("call/check_finite")
def _check_finite():
    f1, f2 = fmaps()
    with torch.no_grad():
        blk = CorrBlock1D(f1, f2, check_finite=True)
        return _block(blk), blk(coords())


def _strided(kind, shape=DEFAULT, **kw):
    """coords that are a view: every other column of a wider tensor, or the
    first two of three channels (another batch stride)."""
    B, _, H, W1, _ = shape
    blk = block(shape, BF16 if kw.get("layout") == "records" else F32, **kw)
    if kind == "columns":
        c = torch.zeros(B, 2, H, 2 * W1, device=DEV)[..., ::2]
    else:
        c = torch.zeros(B, 3, H, W1, device=DEV)[:, :2]
    with torch.no_grad():
        return blk(c), blk.lookup_step(c) if kw.get("layout") != "disparity" else None


for _k in ("columns", "channels"):
    scenario(f"strided/{_k}_L4", _k)(_strided)
    scenario(f"strided/{_k}_L3", _k, num_levels=3)(_strided)
    scenario(f"strided/{_k}_low_latency", _k, low_latency=True)(_strided)
    scenario(f"strided/{_k}_B1", _k, ONE)(_strided)
    scenario(f"strided/{_k}_records", _k, RECORDS, layout="records")(_strided)
    scenario(f"strided/{_k}_disparity", _k, layout="disparity")(_strided)


def _replaced(**kw):
    """A replaced corr_pyramid: the per-level lookup on what was assigned."""
    blk = block(**kw)
    with torch.no_grad():
        full = [t.clone() for t in blk.corr_pyramid]
        blk.corr_pyramid = full
        w, b = convc1(blk)
        return _block(blk), blk(coords()), blk.lookup_step(coords()), blk.lookup_convc1(coords(), w, b)


scenario("replaced/L4")(_replaced)
scenario("replaced/L4_out_f16_channels_last", out_dtype=F16, channels_last=True)(_replaced)
scenario("replaced/disparity", layout="disparity")(_replaced)


@scenario("replaced/records")
def _replaced_records():
    blk = block(RECORDS, BF16, layout="records")
    with torch.no_grad():
        blk.corr_pyramid = list(blk.corr_pyramid)
        return _block(blk), blk(coords(RECORDS))


def _pyramid(shape=DEFAULT, dtype=F32, **kw):
    blk = block(shape, dtype, **kw)
    before = blk.levels_stored
    pyr = blk.corr_pyramid
    return before, pyr, blk.levels_stored, blk.corr_pyramid is pyr


for _n, _a, _kw in (("L4", (), {}), ("L2", (), dict(num_levels=2)), ("L3", (), dict(num_levels=3)),
                    ("L5", (), dict(num_levels=5)), ("low_latency", (), dict(low_latency=True)),
                    ("eager", (), dict(lazy_levels=False)), ("padded_L4", (PADDED,), {}),
                    ("pyr_f16", (), dict(pyramid_dtype=F16)),
                    ("disparity_L4", (), dict(layout="disparity")),
                    ("disparity_L2", (), dict(layout="disparity", num_levels=2)),
                    ("records", (RECORDS, BF16), dict(layout="records")),
                    ("empty_B0", ((0, 32, 3, 40, 40),), {})):
    scenario("corr_pyramid/" + _n, *_a, **_kw)(_pyramid)


@scenario("corr/static")
def _corr_static():
    f1, f2 = fmaps(PADDED)
    with torch.no_grad():
        return (CorrBlock1D.corr(f1, f2), CorrBlock1D.corr(f1, f2, exact_f32=True),
                CorrBlock1D.corr(f1.bfloat16(), f2.bfloat16()))


def _step(shape=DEFAULT, dtype=F32, **kw):
    blk = block(shape, dtype, **kw)
    c = coords(shape)
    delta = torch.full_like(c, 0.25)
    with torch.no_grad():
        first = blk.lookup_step(c)
        second = blk.lookup_step(c, delta)
        third = blk.lookup_step(c, delta, out=c)
        return first, second, third, third[1] is c


for _n, _a, _kw in (("L4", (), {}), ("L2", (), dict(num_levels=2)), ("L3", (), dict(num_levels=3)),
                    ("L5", (), dict(num_levels=5)), ("L4_r5", (), dict(radius=5)),
                    ("low_latency", (), dict(low_latency=True)),
                    ("low_latency_channels_last_out_bf16", (),
                     dict(low_latency=True, channels_last=True, out_dtype=BF16)),
                    ("channels_last_out_f16", (), dict(channels_last=True, out_dtype=F16)),
                    ("L3_channels_last_out_f16", (), dict(num_levels=3, channels_last=True, out_dtype=F16)),
                    ("shadow_true", (), dict(shadow=True)), ("padded_L4", (PADDED,), {}),
                    ("B1_L4", (ONE,), {}), ("pyr_bf16", (), dict(pyramid_dtype=BF16)),
                    ("eager", (), dict(lazy_levels=False)),
                    ("records", (RECORDS, BF16), dict(layout="records")),
                    ("records_channels_last_out_f16", (RECORDS, BF16),
                     dict(layout="records", channels_last=True, out_dtype=F16)),
                    ("empty_B0", ((0, 32, 3, 40, 40),), dict(out_dtype=F16)),
                    ("empty_H0_records", ((1, 256, 0, 72, 72), BF16), dict(layout="records"))):
    scenario("lookup_step/" + _n, *_a, **_kw)(_step)


def _convc1(shape=DEFAULT, dtype=F32, **kw):
    blk = block(shape, dtype, **kw)
    c = coords(shape)
    w, b = convc1(blk)
    before = blk.levels_stored
    with torch.no_grad():
        outs = (blk.lookup_convc1(c, w, b), blk.lookup_convc1(c, w), blk.lookup_convc1(c, w, b, relu=False),
                blk.lookup_convc1(c, w, b, differentiable=True), blk.lookup_convc1(c, w, b, out_dtype=F16),
                blk.lookup_convc1(c, w, out_dtype=BF16, differentiable=True),
                blk.lookup_convc1(c, w.half(), b.half()))
    return before, outs, blk.levels_stored


for _n, _a, _kw in (("L4", (), {}), ("L2", (), dict(num_levels=2)), ("L3", (), dict(num_levels=3)),
                    ("low_latency", (), dict(low_latency=True)),
                    ("shadow_true", (), dict(shadow=True)), ("padded_L4", (PADDED,), {}),
                    ("B1_L4", (ONE,), {}), ("pyr_bf16", (), dict(pyramid_dtype=BF16)),
                    ("out_f16_block", (), dict(out_dtype=F16)), ("eager", (), dict(lazy_levels=False)),
                    ("empty_B0", ((0, 32, 3, 40, 40),), {}),
                    ("empty_H0_L3", ((2, 32, 0, 40, 40),), dict(num_levels=3))):
    scenario("lookup_convc1/" + _n, *_a, **_kw)(_convc1)


def _train(shape=DEFAULT, dtype=F32, calls=3, max_pending=None, fused=False, fmap_grad=True, **kw):
    """One backward() through ``calls`` lookups of one block."""
    if fmap_grad:
        blk, f1, f2 = block(shape, dtype, grad=True, **kw)
    else:
        blk, f1, f2 = block(shape, dtype, **kw), None, None
    if max_pending is not None:
        blk._state.max_pending_calls = max_pending
    w, b = convc1(blk, grad=True)
    loss, outs = 0, []
    for i in range(calls):
        c = coords(shape, seed=i)
        if fused == "out_f16":
            out = blk.lookup_convc1(c, w, b, differentiable=True, out_dtype=F16)
        elif fused == "nobias":
            out = blk.lookup_convc1(c, w, differentiable=True)
        elif fused:
            out = blk.lookup_convc1(c, w, b, differentiable=True)
        else:
            out = blk(c)
        outs.append(out)
        loss = loss + out.float().sum()
    loss.backward()
    return (_block(blk), outs, [o.grad_fn is not None for o in outs], None if f1 is None else f1.grad,
            None if f2 is None else f2.grad,
            w.grad, b.grad)


for _n, _a, _kw in (
        ("deferred_L4", (), {}), ("deferred_L2", (), dict(num_levels=2)),
        ("deferred_partial_flush", (), dict(max_pending=2)),
        ("deferred_partial_flush_5_calls", (), dict(max_pending=2, calls=5)),
        ("grad_shadow_0_2", (), dict(grad_shadow=(0, 2))), ("grad_shadow_2", (), dict(grad_shadow=(2,))),
        ("grad_deferred_false", (), dict(grad_deferred=False)),
        ("L3", (), dict(num_levels=3)), ("L5", (), dict(num_levels=5)), ("L4_r5", (), dict(radius=5)),
        ("low_latency", (), dict(low_latency=True)), ("exact_f32", (), dict(exact_f32=True)),
        ("padded_L4", (PADDED,), {}), ("B1_L4", (ONE,), {}), ("out_f16", (), dict(out_dtype=F16)),
        ("bf16_fmaps", (DEFAULT, BF16), {}), ("f16_fmaps_f16_pyramid", (DEFAULT, F16), dict(pyramid_dtype=F16)),
        ("disparity", (), dict(layout="disparity")),
        ("records", (RECORDS, BF16), dict(layout="records")),
        ("records_grad_deferred_false", (RECORDS, BF16), dict(layout="records", grad_deferred=False)),
        ("fused_L4", (), dict(fused=True)), ("fused_L2_nobias", (), dict(fused="nobias", num_levels=2)),
        ("fused_L3", (), dict(fused=True, num_levels=3)), ("fused_out_f16", (), dict(fused="out_f16")),
        ("fused_low_latency", (), dict(fused=True, low_latency=True)),
        ("fused_shadow_true_padded", (PADDED,), dict(fused=True, shadow=True)),
        ("fused_weights_only_L4", (), dict(fused=True, fmap_grad=False)),
        ("fused_weights_only_L3", (), dict(fused=True, fmap_grad=False, num_levels=3)),
        ("fused_grad_deferred_false", (), dict(fused=True, grad_deferred=False))):
    scenario("backward/" + _n, *_a, **_kw)(_train)


@scenario("backward/no_lookup_reaches_loss")
def _train_nothing():
    blk, f1, f2 = block(grad=True)
    (blk._token * 1.0).backward()
    return f1.grad, f2.grad


@scenario("backward/two_graphs")
def _train_twice():
    blk, f1, f2 = block(grad=True)
    blk(coords()).sum().backward(retain_graph=True)
    blk(coords()).sum().backward()
    return f1.grad, f2.grad


def _every_other(t):
    """The same level with a row stride of 2 elements: the glue has to copy it
    (and then drops the shadow flags, the copy has no shadow)."""
    v = torch.empty(t.shape[:-1] + (2 * t.shape[-1],), dtype=t.dtype, device=t.device)[..., ::2]
    v.copy_(t)
    return v


@scenario("functions/lookups")
def _functions():
    """The module-level functions tests and tools call on a pyramid list."""
    with torch.no_grad():
        f1, f2 = fmaps(PADDED)
        full = rcorr.build_pyramid(f1, f2, 5)
        plain = rcorr.build_pyramid(f1, f2, 3, pad=False)
        pair = rcorr.build_pyramid(f1, f2, 3, skip=(1,), shadow=(2,))
        c = coords(PADDED)
        wide, cw = rcorr.build_pyramid(*fmaps(), 1, shadow=True), coords()
        return (full, plain, pair, rcorr.lookup(full, c, 4, 4), rcorr.lookup(plain, c, 3, 2),
                rcorr.lookup_chain(full, c, 4, 4), rcorr.lookup_chain(full, c, 3, 4),
                rcorr.lookup_chain(pair, c, 4, 4, shadow=(2,), channels_last=True, out_dtype=F16),
                rcorr.lookup_chain(pair, c, 4, 4, shadow=True),
                rcorr.lookup_chain(full[:2], c, 3, 3, channels_last=True, out_dtype=BF16),
                rcorr.lookup_chain([full[0]], c, 2, 4),
                rcorr.lookup_chain([_every_other(wide[0])], cw, 2, 4, shadow=True),
                rcorr.pool_level(full[0]), rcorr.pool_level(plain[1]))


@scenario("functions/records")
def _functions_records():
    with torch.no_grad():
        blk = block(RECORDS, BF16, layout="records")
        rec, c = blk._records, coords(RECORDS)
        args = rcorr._records_args(rec, 72)
        return (rcorr.lookup_records(rec, c, 4, 72), rcorr.lookup_records(rec, c, 3, 72, True, F16),
                [list(a) == list(b) for a, b in zip(args[1:], ([72, 36, 18, 9],) * 2)],
                rcorr.records_level(rec, 0, 72), rcorr.records_level(rec, 2, 72))


@scenario("functions/gradients")
def _functions_gradients():
    B, D, H, W1, W2 = PADDED
    P, widths = B * H * W1, [W2 >> l for l in range(4)]
    c = coords(PADDED)
    go = torch.ones(B, 36, H, W1, device=DEV)
    f1, f2 = fmaps(PADDED)
    out = []
    for kw in (dict(), dict(pair=True), dict(pair=True, shadow=(0, 2)), dict(pair=True, zero=False)):
        g = rcorr.grad_buffers(P, widths, DEV, **kw)
        if kw.get("zero", True):
            rcorr.lookup_backward(g, c, go, 4, 4)
        if not kw.get("shadow"):
            rcorr.lookup_backward_calls(g, [c, c], [go, go.half()], 4, 4, overwrite=not kw.get("zero", True))
            rcorr.lookup_backward_calls(g, [], [], 4, 4)
            rcorr.lookup_backward_calls(g, [], [], 4, 4, overwrite=True)
        out.append((g, sorted(g.shadow), rcorr.build_backward(f1, f2, g),
                    rcorr.build_backward(f1.half(), f2.bfloat16(), g, exact_f32=True)))
    g2 = rcorr.grad_buffers(P, widths[:2], DEV, pair=True)
    rcorr.lookup_backward(g2, c, go[:, :18], 2, 4)
    out.append((g2, rcorr.build_backward(f1, f2, g2)))
    e1, e2 = fmaps((0, 32, 3, 40, 37))
    out.append(rcorr.build_backward(e1, e2, rcorr.grad_buffers(0, widths, DEV)))
    rcorr.lookup_backward(rcorr.grad_buffers(0, widths, DEV), c[:0], go[:0], 4, 4)
    rcorr.lookup_backward_calls(rcorr.grad_buffers(0, widths, DEV, pair=True), [c[:0]], [go[:0]], 4, 4)
    return out


@scenario("functions/convc1")
def _functions_convc1():
    """The four fused-conv functions on pyramid lists, every need_* subset."""
    with torch.no_grad():
        blk = block(PADDED, shadow=True)
        full = blk.corr_pyramid
        pair = [full[0], None, full[2], None]
        c = coords(PADDED)
        w, b = convc1(blk)
        go = torch.ones(2, 8, 3, 40, device=DEV)
        out = [rcorr.lookup_convc1(full, c, 4, 4, w, b), rcorr.lookup_convc1(full, c, 3, 4, w[:, :27], relu=False),
               rcorr.lookup_chain_convc1(pair, c, 4, 4, w, b, shadow=blk._shadow, out_dtype=BF16),
               rcorr.lookup_chain_convc1(full[:1], c, 2, 4, w[:, :18])]
        for need in ((True, True, True), (True, False, False), (False, True, False), (False, False, True),
                     (False, False, False)):
            out.append(rcorr.lookup_convc1_backward(full, c, 4, 4, w, b, True, go, *need))
            out.append(rcorr.lookup_chain_convc1_backward(pair, c, 4, 4, w, b, True, go.half(), *need,
                                                          shadow=blk._shadow))
        out.append(rcorr.lookup_convc1_backward(full, c, 4, 4, w, None, False, go, need_bias=False))
        out.append(rcorr.lookup_chain_convc1_backward(pair, c, 4, 4, w, None, False, go, need_bias=False))
        empty = block((0, 32, 3, 40, 37)).corr_pyramid
        out.append(rcorr.lookup_convc1_backward(empty, c[:0], 4, 4, w, b, True, go[:0]))
        out.append(rcorr.lookup_chain_convc1_backward(empty[:3], c[:0], 4, 4, w, b, True, go[:0],
                                                      need_weight=False))
        return out


# -- refusals: one per raising branch of the glue (the exception is the trace)

def _refuse_coords(what, method="call", shape=DEFAULT, dtype=F32, **kw):
    blk = block(shape, dtype, **kw)
    c = coords(shape)
    bad = {"dtype": c.double(), "rank": c[0], "rows": c[..., :-1], "cpu": c.cpu(), "channels": c[:, :0],
           "type": None}[what]
    with torch.no_grad():
        if method == "call":
            return blk(bad)
        if method == "step":
            return blk.lookup_step(bad)
        return blk.lookup_convc1(bad, *convc1(blk))


for _what in ("dtype", "rank", "rows", "cpu", "channels", "type"):
    for _n, _a, _kw in (("rows_L4", (), {}), ("rows_L3", (), dict(num_levels=3)),
                        ("low_latency", (), dict(low_latency=True)),
                        ("records", (RECORDS, BF16), dict(layout="records")),
                        ("disparity", (), dict(layout="disparity"))):
        scenario(f"refuse/coords_{_what}/call_{_n}", _what, "call", *_a, **_kw)(_refuse_coords)
    for _n, _a, _kw in (("rows_L4", (), {}), ("records", (RECORDS, BF16), dict(layout="records"))):
        scenario(f"refuse/coords_{_what}/step_{_n}", _what, "step", *_a, **_kw)(_refuse_coords)
    for _n, _a, _kw in (("rows_L4", (), {}), ("rows_L3", (), dict(num_levels=3))):
        scenario(f"refuse/coords_{_what}/convc1_{_n}", _what, "convc1", *_a, **_kw)(_refuse_coords)


def _refuse_convc1(what, **kw):
    blk = block(**kw)
    c = coords()
    w, b = convc1(blk)
    with torch.no_grad():
        if what == "cin":
            return blk.lookup_convc1(c, w[:, :-1], b)
        if what == "bias_len":
            return blk.lookup_convc1(c, w, b[:-1])
        if what == "weight_cpu":
            return blk.lookup_convc1(c, w.cpu(), b)
        if what == "bias_cpu":
            return blk.lookup_convc1(c, w, b.cpu())
        if what == "weight_type":
            return blk.lookup_convc1(c, None, b)
        if what == "out_dtype":
            return blk.lookup_convc1(c, w, b, out_dtype=torch.float64)
    levels = blk._levels if blk.num_levels == 4 else blk._read_levels()
    bwd = rcorr.lookup_chain_convc1_backward if blk.num_levels == 4 else rcorr.lookup_convc1_backward
    go = torch.ones(2, 8, 3, 40, device=DEV)
    if what == "bwd_grad_out":
        return bwd(levels, c, blk.num_levels, 4, w, b, True, go[:, :-1])
    if what == "bwd_cin":
        return bwd(levels, c, blk.num_levels, 4, w[:, :-1], b, True, go)
    if what == "bwd_coords":
        return bwd(levels, c.double(), blk.num_levels, 4, w, b, True, go)
    # weight and bias of the backwards go through the forward's checks: one on
    # another device is refused, not handed to the kernel as a foreign pointer
    if what == "bwd_weight_cpu":
        return bwd(levels, c, blk.num_levels, 4, w.cpu(), b, True, go)
    if what == "bwd_bias_cpu":
        return bwd(levels, c, blk.num_levels, 4, w, b.cpu(), True, go)
    if what == "bwd_bias_len":
        return bwd(levels, c, blk.num_levels, 4, w, b[:-1], True, go)
    raise AssertionError(what)


for _what in ("cin", "bias_len", "weight_cpu", "bias_cpu", "weight_type", "out_dtype", "bwd_grad_out", "bwd_cin",
              "bwd_coords", "bwd_weight_cpu", "bwd_bias_cpu", "bwd_bias_len"):
    scenario(f"refuse/convc1_{_what}/pair")(lambda w=_what: _refuse_convc1(w))
    scenario(f"refuse/convc1_{_what}/per_level")(lambda w=_what: _refuse_convc1(w, num_levels=3))


@scenario("refuse/convc1_chain_not_pair")
def _refuse_chain_not_pair():
    blk = block(num_levels=3)
    w, b = convc1(blk)
    return rcorr.lookup_chain_convc1(blk._levels, coords(), 3, 4, w, b)


@scenario("refuse/convc1_chain_backward_not_pair")
def _refuse_chain_backward_not_pair():
    blk = block(num_levels=3)
    w, b = convc1(blk)
    return rcorr.lookup_chain_convc1_backward(blk._levels, coords(), 3, 4, w, b, True,
                                              torch.ones(2, 8, 3, 40, device=DEV))


def _refuse_method(method, shape=DEFAULT, dtype=F32, grad=False, **kw):
    blk = block(shape, dtype, grad=grad, **kw)
    blk = blk[0] if grad else blk
    c = coords(shape)
    w, b = convc1(blk, grad=method == "convc1_weight_grad")
    if method == "step":
        with torch.no_grad():
            return blk.lookup_step(c)
    if method == "step_grad":
        return blk.lookup_step(c)
    if method == "convc1":
        with torch.no_grad():
            return blk.lookup_convc1(c, w, b)
    if method == "convc1_diff":
        with torch.no_grad():
            return blk.lookup_convc1(c, w, b, differentiable=True)
    return blk.lookup_convc1(c, w, b)           # under grad, not differentiable


scenario("refuse/step_disparity", "step", layout="disparity")(_refuse_method)
scenario("refuse/step_f16_pyramid", "step", pyramid_dtype=F16)(_refuse_method)
scenario("refuse/step_under_grad", "step_grad", grad=True)(_refuse_method)
scenario("refuse/convc1_records", "convc1", RECORDS, BF16, layout="records")(_refuse_method)
scenario("refuse/convc1_records_differentiable", "convc1_diff", RECORDS, BF16, layout="records")(_refuse_method)
scenario("refuse/convc1_disparity", "convc1", layout="disparity")(_refuse_method)
scenario("refuse/convc1_f16_pyramid", "convc1", pyramid_dtype=F16)(_refuse_method)
scenario("refuse/convc1_L5", "convc1", num_levels=5)(_refuse_method)       # the C side's refusal
scenario("refuse/convc1_under_grad", "convc1_grad", grad=True)(_refuse_method)
scenario("refuse/convc1_weight_grad", "convc1_weight_grad")(_refuse_method)


def _refuse_step(what):
    blk = block()
    c = coords()
    d = torch.zeros_like(c)
    with torch.no_grad():
        if what == "channels":
            return blk.lookup_step(torch.zeros(2, 1, 3, 40, device=DEV))
        if what == "delta_cpu":
            return blk.lookup_step(c, d.cpu())
        if what == "delta_shape":
            return blk.lookup_step(c, d[..., :-1])
        if what == "out_cpu":
            return blk.lookup_step(c, d, out=c.cpu())
        if what == "out_dtype":
            return blk.lookup_step(c, d, out=c.double())
        if what == "out_strided":
            return blk.lookup_step(c, d, out=torch.zeros(2, 2, 3, 80, device=DEV)[..., ::2])
    raise AssertionError(what)


for _what in ("channels", "delta_cpu", "delta_shape", "out_cpu", "out_dtype", "out_strided"):
    scenario("refuse/step_" + _what, _what)(_refuse_step)


def _refuse_ctor(shape=DEFAULT, dtype=F32, **kw):
    return _block(block(shape, dtype, **kw))


for _n, _a, _kw in (
        ("layout_name", (), dict(layout="sheared")), ("out_dtype", (), dict(out_dtype=torch.float64)),
        ("too_narrow", (), dict(num_levels=6)), ("zero_levels", (), dict(num_levels=0)),
        ("grad_shadow_level", (), dict(grad_shadow=(1,))), ("grad_shadow_L3", (), dict(grad_shadow=(0,), num_levels=3)),
        ("disparity_L3", (), dict(layout="disparity", num_levels=3)),
        ("disparity_bf16", (DEFAULT, BF16), dict(layout="disparity")),
        ("disparity_channels_last", (), dict(layout="disparity", channels_last=True)),
        ("disparity_low_latency", (), dict(layout="disparity", low_latency=True)),
        ("disparity_eager", (), dict(layout="disparity", lazy_levels=False)),
        ("disparity_exact_f32", (), dict(layout="disparity", exact_f32=True)),
        ("disparity_width", ((2, 32, 3, 38, 40),), dict(layout="disparity")),
        ("records_f32", (RECORDS,), dict(layout="records", pyramid_dtype=F32)),
        ("records_L2", (RECORDS, BF16), dict(layout="records", num_levels=2)),
        ("records_narrow", ((1, 256, 2, 64, 64), BF16), dict(layout="records")),
        ("records_low_latency", (RECORDS, BF16), dict(layout="records", low_latency=True)),
        ("records_shadow", (RECORDS, BF16), dict(layout="records", shadow=True)),
        ("records_grad_shadow", (RECORDS, BF16), dict(layout="records", grad_shadow=(0,))),
        ("records_eager", (RECORDS, BF16), dict(layout="records", lazy_levels=False)),
        ("f16_pyramid_records", (), dict(layout="records", pyramid_dtype=F16)),
        ("f16_pyramid_exact_f32", (), dict(exact_f32=True, pyramid_dtype=F16)),
        ("f16_pyramid_bf16_fmaps", (DEFAULT, BF16), dict(pyramid_dtype=F16)),
        ("fmap_dtype", (DEFAULT, torch.float64), {})):
    scenario("refuse/ctor_" + _n, *_a, **_kw)(_refuse_ctor)


@scenario("refuse/ctor_fmap_shapes")
def _refuse_fmap_shapes():
    f1, f2 = fmaps()
    return CorrBlock1D(f1, f2[:, :, :2])


@scenario("refuse/ctor_fmap_cpu")
def _refuse_fmap_cpu():
    f1, f2 = fmaps()
    return CorrBlock1D(f1, f2.cpu())


def _refuse_gradients(what):
    B, D, H, W1, W2 = DEFAULT
    widths = [W2 >> l for l in range(4)]
    c = coords()
    go = torch.ones(B, 36, H, W1, device=DEV)
    g = rcorr.grad_buffers(B * H * W1, widths, DEV, pair=True, shadow=(0,) if what == "calls_shadow" else ())
    if what == "buffers_shadow":
        return rcorr.grad_buffers(B * H * W1, widths, DEV, shadow=(0,))
    if what == "grad_out":
        return rcorr.lookup_backward(g, c, go[:, :-1], 4, 4)
    if what == "coords_dtype":
        return rcorr.lookup_backward(g, c.double(), go, 4, 4)
    if what == "coords_rows":
        return rcorr.lookup_backward(g, c[..., :-1], go[..., :-1], 4, 4)
    if what == "coords_cpu":
        return rcorr.lookup_backward(g, c.cpu(), go, 4, 4)
    if what == "calls_count":
        return rcorr.lookup_backward_calls(g, [c, c], [go], 4, 4)
    if what == "calls_shadow":
        return rcorr.lookup_backward_calls(g, [c], [go], 4, 4)
    if what == "calls_grad_out":
        return rcorr.lookup_backward_calls(g, [c, c], [go, go[:, :-1]], 4, 4)
    if what == "calls_coords_rows":
        return rcorr.lookup_backward_calls(g, [c, c[..., :-1]], [go, go[..., :-1]], 4, 4)
    if what == "calls_coords_shape":
        return rcorr.lookup_backward_calls(g, [c, c.reshape(B, 2, W1, H)], [go, go.reshape(B, 36, W1, H)], 4, 4)
    raise AssertionError(what)


for _what in ("buffers_shadow", "grad_out", "coords_dtype", "coords_rows", "coords_cpu", "calls_count",
              "calls_shadow", "calls_grad_out", "calls_coords_rows", "calls_coords_shape"):
    scenario("refuse/gradients_" + _what, _what)(_refuse_gradients)


@scenario("refuse/chain_mixed_dtypes")
def _refuse_mixed():
    with torch.no_grad():
        pyr = block()._levels
        return rcorr.lookup_chain([pyr[0], None, pyr[2].bfloat16(), None], coords(), 4, 4)


@scenario("refuse/pyramid_rows_strided")
def _refuse_rows_strided():
    with torch.no_grad():
        pyr = block().corr_pyramid
        return rcorr.pool_level(pyr[0][..., ::2])


@scenario("refuse/two_faults_chain_convc1")
def _refuse_two_chain_convc1():
    """Bad coords and no pair layout: the coords are refused first."""
    blk = block(num_levels=3)
    w, b = convc1(blk)
    return rcorr.lookup_chain_convc1(blk._levels, coords().double(), 3, 4, w, b)


@scenario("refuse/two_faults_chain_convc1_backward")
def _refuse_two_chain_convc1_backward():
    blk = block(num_levels=3)
    w, b = convc1(blk)
    return rcorr.lookup_chain_convc1_backward(blk._levels, coords().double(), 3, 4, w, b, True,
                                              torch.ones(2, 8, 3, 40, device=DEV))


@scenario("refuse/two_faults_lookup_chain")
def _refuse_two_lookup_chain():
    """Bad coords and a bad out_dtype: the coords are refused first."""
    with torch.no_grad():
        return rcorr.lookup_chain(block()._levels, coords().double(), 4, 4, out_dtype=torch.float64)


@scenario("refuse/pool_level_cpu")
def _refuse_pool_cpu():
    """pool_level and build_backward do not check their tensors' device: the
    launch does."""
    return rcorr.pool_level(torch.zeros(8, 1, 1, 16))


@scenario("refuse/build_backward_cpu")
def _refuse_build_backward_cpu():
    f = torch.zeros(1, 8, 2, 16)
    return rcorr.build_backward(f, f, rcorr.grad_buffers(32, [16, 8], "cpu"))


# --------------------------------------------------------- record / compare

def _run(fn):
    rec = _Recorder(_lib.lib())
    prev, _lib._active = _lib._active, rec
    try:
        try:
            entry = {"returns": _desc(fn())}
        except Exception as e:          # the refusals: class and message are the trace
            entry = {"raises": [type(e).__name__, str(e)]}
        torch.cuda.synchronize()
    finally:
        _lib._active = prev
    entry["calls"] = rec.calls
    return json.loads(json.dumps(entry))


def _dump(traces, path):
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join(f" {json.dumps(k)}: {json.dumps(traces[k])}" for k in sorted(traces))
                + "\n}\n")


@pytest.fixture(scope="module")
def golden():
    if REGEN:
        traces = {name: _run(fn) for name, fn in SCENARIOS.items()}
        _dump(traces, FIXTURE if REGEN == "1" else REGEN)
        return traces
    with open(FIXTURE) as f:
        return json.load(f)


def test_fixture_covers_every_scenario(golden):
    assert sorted(golden) == sorted(SCENARIOS)


def _first_difference(want, got):
    for key in ("raises", "returns"):
        if want.get(key) != got.get(key):
            return f"{key}: fixture {want.get(key)!r}\n{' ' * len(key)}  now     {got.get(key)!r}"
    for i, (a, b) in enumerate(zip(want["calls"], got["calls"])):
        if a != b:
            return f"call {i}: fixture {a!r}\n{' ' * len(str(i))}       now     {b!r}"
    n = min(len(want["calls"]), len(got["calls"]))
    extra = (want["calls"] + got["calls"])[n:n + 1]
    return f"fixture has {len(want['calls'])} calls, now {len(got['calls'])}; first unmatched: {extra!r}"


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_glue_trace(golden, name):
    got = _run(SCENARIOS[name])
    want = golden[name]
    if got != want:
        diff = _first_difference(want, got)
        print(f"{name}: {diff}")
        pytest.fail(f"{name}: the glue's C-ABI trace moved\n{diff}", pytrace=False)
