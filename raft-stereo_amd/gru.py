"""The ConvGRU update with its elementwise glue on two gfx950 kernels
(rc_gru_gates, rc_gru_blend; csrc/gru_gates.hip).

``ConvGRU.forward`` (network.py) is three convolutions surrounded by two
concatenations and about eleven elementwise launches.  ``conv_gru_forward``
keeps the convolutions where they are and runs the rest as

  1. one ``torch.cat`` of h and every part of x into the [h, x] buffer,
  2. convz and convr as one stacked convolution (``_zr_conv``),
  3. ``gru_gates``: z in place on the convolution output, r*h over the first
     C channels of the [h, x] buffer, which thereby becomes [r*h, x],
  4. convq on that buffer,
  5. ``gru_blend``: the new hidden state.

It is opt-in (``ConvGRU.fuse``, ``RAFTStereo(fuse_gru=True)``) and has no CPU
fallback: the wrappers raise on tensors that are not on a HIP device.  With a
gradient being recorded ``fusable`` is false and the PyTorch ops run, unless
the training route is asked for as well (``ConvGRU.fuse_backward``,
``RAFTStereo(fuse_gru_backward=True)``,
``conv_gru_forward(differentiable=True)``): the same kernels inside two
``torch.autograd.Function``s whose backward is one launch each
(rc_gru_gates_backward, rc_gru_blend_backward; csrc/gru_gates_bwd.hip), the
convolutions and the concatenations ordinary autograd ops.  That route keeps
the [h, x] buffer, which the first convolution saves, and concatenates
[r*h, x] into a second one.

The work in front of each call -- ``pool2x`` / ``interp`` of the neighbouring
scales' states and the concatenation itself -- can join the inference route
as one more launch (rc_gru_assemble; csrc/gru_inputs.hip): the caller hands
``Pooled(src)`` / ``Resized(src, size)`` descriptors instead of the pooled /
resized tensors, and with ``ConvGRU.fuse_inputs`` set
(``RAFTStereo(fuse_gru_inputs=True)``) ``assemble`` fills the [h, x] buffer
from h, the plain parts and the descriptors' sources, where all of them are
in the buffer's memory format.  Every other route materialises the
descriptors with the PyTorch ops first and runs as before.

The training route does the same with ``ConvGRU.fuse_inputs_backward`` set
(``RAFTStereo(fuse_gru_inputs_backward=True)``): [h, x] and [r*h, x] are one
``assemble`` launch each inside two more ``torch.autograd.Function``s, and
the gradients of h and of every part's source come from one launch of the
assembly's adjoint (rc_gru_assemble_backward; csrc/gru_inputs_bwd.hip,
``assemble_backward``) instead of the backward of two concatenations, the
casts, ``avg_pool2d``, ``interpolate`` and an accumulation add per part.
"""
import weakref

import torch
import torch.nn.functional as F

from . import _lib

_CODES = {torch.float32: _lib.RC_F32, torch.float16: _lib.RC_F16, torch.bfloat16: _lib.RC_BF16}

_ZR = weakref.WeakKeyDictionary()   # ConvGRU -> (weight, bias, C, tag): convz and convr stacked
_ZR_CAST = weakref.WeakKeyDictionary()   # ConvGRU -> (stacked weight, dtype, weight cast, bias cast)


_MODES = {"copy": _lib.RC_PART_COPY, "pool2x": _lib.RC_PART_POOL2X, "bilinear": _lib.RC_PART_BILINEAR}


class _Lazy:
    """A part of x that has not been computed yet: what ``assemble`` needs to
    compute it (``src``, ``mode``) and what the checks need of the result."""
    mode = None

    def __init__(self, src):
        if not isinstance(src, torch.Tensor) or src.dim() != 4:
            raise TypeError(f"{type(self).__name__}: a 4-D tensor, not {type(src).__name__}")
        self.src = src

    dtype = property(lambda self: self.src.dtype)
    device = property(lambda self: self.src.device)
    requires_grad = property(lambda self: self.src.requires_grad)

    def dim(self):
        return 4

    def size(self, d=None):
        return self.shape if d is None else self.shape[d]


class Pooled(_Lazy):
    """``network.pool2x(src)``, not computed yet."""
    mode = "pool2x"

    @property
    def shape(self):
        N, C, H, W = self.src.shape
        return torch.Size((N, C, (H - 1) // 2 + 1, (W - 1) // 2 + 1))

    def materialize(self):
        from . import network
        return network.pool2x(self.src)


class Resized(_Lazy):
    """``network.interp(src, dest)`` with ``size = dest.shape[2:]``, not computed yet."""
    mode = "bilinear"

    def __init__(self, src, size):
        super().__init__(src)
        self.out_size = tuple(int(v) for v in size)
        if len(self.out_size) != 2:
            raise ValueError(f"Resized: size {size!r}: (H, W)")

    @property
    def shape(self):
        return torch.Size((*self.src.shape[:2], *self.out_size))

    def materialize(self):
        from . import network
        # interp reads its second argument's spatial size only
        return network.interp(self.src, torch.empty((0, 0, *self.out_size), device="meta"))


def materialized(x_list):
    """x_list with every descriptor replaced by its tensor (the PyTorch ops)."""
    return tuple(x.materialize() if isinstance(x, _Lazy) else x for x in x_list)


def _is_part(t):
    return isinstance(t, (torch.Tensor, _Lazy))


def _zr_conv(gru):
    """convz and convr as ONE conv (weights stacked along the output channels):
    the same per-channel sums, one launch instead of two and no sliced input
    for convz -- at 60-row slabs each launch's fixed cost matters (DESIGN.md
    §5).  Cached per module only while no gradient is recorded (a cached
    autograd node could not be back-propagated twice); the cache entry is
    keyed on each weight's storage, in-place version, dtype and device, so
    ``.to()`` / ``.double()`` / ``load_state_dict`` (which keep the Parameter
    object) rebuild it."""
    wz, wr = gru.convz.weight, gru.convr.weight
    bz, br = gru.convz.bias, gru.convr.bias
    ws = [t for t in (wz, wr, bz, br) if t is not None]
    if torch.is_grad_enabled() and any(t.requires_grad for t in ws):
        w = torch.cat([wz, wr], 0)
        return w, (None if bz is None else torch.cat([bz, br], 0)), wz.shape[0]
    tag = tuple((t.data_ptr(), t._version, t.dtype, t.device) for t in ws)
    hit = _ZR.get(gru)
    if hit is None or hit[3] != tag:
        w = torch.cat([wz, wr], 0)
        b = None if bz is None else torch.cat([bz, br], 0)
        hit = _ZR[gru] = (w, b, wz.shape[0], tag)
    return hit[0], hit[1], hit[2]


def _zr_conv_as(gru, dtype):
    """``_zr_conv`` in ``dtype`` (no gradient recorded): under autocast the
    stacked weights are no leaf, so autocast's own cast cache would convert
    them at every call; the cast is kept with the entry it was made from."""
    w, b, C = _zr_conv(gru)
    if w.dtype == dtype:
        return w, b, C
    hit = _ZR_CAST.get(gru)
    if hit is None or hit[0] is not w or hit[1] != dtype:
        hit = _ZR_CAST[gru] = (w, dtype, w.to(dtype), None if b is None else b.to(dtype))
    return hit[2], hit[3], C


def _triple(t):
    """(batch, channel, pixel) strides in elements of a 4-D tensor whose H and
    W merge into one pixel axis, else None."""
    _, _, H, W = t.shape
    sn, sc, sh, sw = t.stride()
    if H == 1:
        return sn, sc, (1 if W == 1 else sw)
    if W == 1:
        return sn, sc, sh
    return (sn, sc, sw) if sh == W * sw else None


def _classes(t):
    """The layout classes a tensor fits: subset of {'planar', 'interleaved'}."""
    tr = _triple(t)
    if tr is None:
        return set()
    _, C, H, W = t.shape
    out = set()
    if H * W <= 1 or tr[2] == 1:
        out.add("planar")
    if C == 1 or tr[1] == 1:
        out.add("interleaved")
    return out


def _common_class(tensors):
    cls = {"planar", "interleaved"}
    for t in tensors:
        cls &= _classes(t)
    return cls


def _compute_dtype(gru, h):
    """The dtype the gate convolutions compute and return in: autocast's on a
    HIP tensor inside an autocast region, else the weights'."""
    if h.device.type == "cuda" and torch.is_autocast_enabled():
        return torch.get_autocast_dtype("cuda")
    return gru.convz.weight.dtype


def why_not_fusable(gru, h, cz, cr, cq, *x_list, differentiable=False):
    """None when ``conv_gru_forward`` can stand in for ``ConvGRU.forward`` on
    these arguments, else the first reason why not, in words.
    ``differentiable``: for ``conv_gru_forward(differentiable=True)``, which
    a gradient being recorded does not stop; every other condition holds.
    A part of x may be a ``Pooled`` / ``Resized`` descriptor: it counts with
    its result's shape and dtype."""
    state = (h, cz, cr, cq)
    tensors = state + tuple(x_list)
    if not x_list or any(not isinstance(t, torch.Tensor) for t in state) or \
            any(not _is_part(t) or t.dim() != 4 for t in tensors):
        return "h, cz, cr, cq and at least one part of x, all 4-D tensors"
    dt = h.dtype
    if dt not in _CODES:
        return f"dtype {dt}: float32, float16 or bfloat16"
    if any(t.dtype != dt for t in state):
        return "h, cz, cr and cq of mixed dtypes"
    autocast = h.device.type == "cuda" and torch.is_autocast_enabled()
    if dt != _compute_dtype(gru, h):
        return f"h is {dt}, the gate convolutions compute in {_compute_dtype(gru, h)}"
    # under autocast the convolution casts its input, so the parts of x may be
    # of another float dtype (the motion features carry the fp32 flow)
    if any(t.dtype != dt and not (autocast and t.dtype in _CODES) for t in x_list):
        return "x parts of mixed dtypes outside autocast"
    if any(t.shape != h.shape for t in state) or any(t.shape[0] != h.shape[0] or t.shape[2:] != h.shape[2:]
                                                       for t in x_list):
        return "shapes do not match h's"
    cz_, cr_, cq_ = gru.convz, gru.convr, gru.convq
    if torch.is_grad_enabled() and not differentiable:
        params = [p for c in (cz_, cr_, cq_) for p in (c.weight, c.bias) if p is not None]
        if any(t.requires_grad for t in tensors) or any(p.requires_grad for p in params):
            return "a gradient is being recorded (there is no backward kernel)"
    if h.device.type != "cuda":
        return f"h is on {h.device}: HIP devices only"
    if any(t.device != h.device for t in tensors) or cz_.weight.device != h.device:
        return "tensors on different devices"
    if not _common_class(state):
        return "h, cz, cr and cq share no layout class with a mergeable H*W"
    if any(type(c) is not torch.nn.Conv2d for c in (cz_, cr_, cq_)):
        return "gates that are not nn.Conv2d"
    geom = [(c.kernel_size, c.stride, c.padding, c.dilation, c.groups, c.padding_mode, c.bias is None)
            for c in (cz_, cr_)]
    if geom[0] != geom[1] or cz_.stride != (1, 1) or cz_.groups != 1 or cz_.padding_mode != "zeros":
        return "convz and convr cannot be stacked"
    if cz_.weight.shape[0] != h.shape[1]:
        return "convz does not return h's channels"
    return None


def fusable(gru, h, cz, cr, cq, *x_list, differentiable=False):
    """Whether ``conv_gru_forward`` can stand in for ``ConvGRU.forward`` on
    these arguments: every tensor on one HIP device; h, cz, cr and cq of one
    dtype out of fp32 / fp16 / bf16, the one the gate convolutions compute in
    (the parts of x may be of other float dtypes only under autocast, where
    the convolution would cast them anyway); h, cz, cr and cq of one layout
    class with a mergeable H*W; convz and convr of one geometry; and no
    gradient being recorded for any input or gate weight -- the last one
    only without ``differentiable``."""
    return why_not_fusable(gru, h, cz, cr, cq, *x_list, differentiable=differentiable) is None


def _check(name, ops, names):
    first = ops[0]
    for t, n in zip(ops, names):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name}: {n} must be a torch.Tensor")
        if t.device.type != "cuda":
            raise RuntimeError(f"{name}: {n} is on {t.device}; the kernel runs on HIP devices only "
                               "(no CPU fallback)")
        if t.device != first.device:
            raise RuntimeError(f"{name}: {n} is on {t.device}, {names[0]} on {first.device}")
        if t.dtype != first.dtype:
            raise ValueError(f"{name}: {n} is {t.dtype}, {names[0]} is {first.dtype}: one dtype for all operands")
        if t.dim() != 4 or t.shape != first.shape:
            raise ValueError(f"{name}: {n} has shape {tuple(t.shape)}, {names[0]} has {tuple(first.shape)}")
    if first.dtype not in _CODES:
        raise ValueError(f"{name}: dtype {first.dtype}: float32, float16 or bfloat16")
    triples = []
    for t, n in zip(ops, names):
        tr = _triple(t)
        if tr is None:
            raise ValueError(f"{name}: H and W of {n} do not merge into one pixel axis (strides {t.stride()})")
        triples += tr
    return _lib.long_array(triples)


def _empty_like_class(ref, cls):
    fmt = torch.channels_last if "planar" not in cls else torch.contiguous_format
    return torch.empty(ref.shape, dtype=ref.dtype, device=ref.device, memory_format=fmt)


def _launch(name, ops, names):
    """``_check`` and the call of entry point rc_<name> on the operands'
    device and current stream."""
    strides = _check(name, ops, names)
    h = ops[0]
    N, C, H, W = h.shape
    with torch.cuda.device(h.device):
        stream = torch.cuda.current_stream(h.device).cuda_stream or None
        rc = getattr(_lib.lib(), "rc_" + name)(*(t.data_ptr() for t in ops), strides, _CODES[h.dtype], N, C, H * W,
                                               stream)
    _lib.check(rc, "rc_" + name)


def gru_gates(z_pre, r_pre, cz, cr, h, z_out=None, rh_out=None):
    """z = sigmoid(z_pre + cz) and r*h with r = sigmoid(r_pre + cr), one launch
    (rc_gru_gates).  All operands (N, C, H, W) of one dtype and one layout
    class; any of them may be a channel slice of a larger tensor.  ``z_out``
    may be ``z_pre``; ``rh_out`` must not be ``h``.  Missing outputs are
    allocated.  Returns (z_out, rh_out)."""
    cls = _common_class((z_pre, r_pre, cz, cr, h))
    if z_out is None:
        z_out = _empty_like_class(h, cls)
    if rh_out is None:
        rh_out = _empty_like_class(h, cls)
    _launch("gru_gates", (z_pre, r_pre, cz, cr, h, z_out, rh_out),
            ("z_pre", "r_pre", "cz", "cr", "h", "z_out", "rh_out"))
    return z_out, rh_out


def gru_blend(z, q_pre, cq, h, h_out=None):
    """h_out = (1 - z) * h + z * tanh(q_pre + cq), one launch (rc_gru_blend).
    Operands as for ``gru_gates``; ``h_out`` may be ``h`` and is allocated
    when missing.  Returns h_out."""
    if h_out is None:
        h_out = _empty_like_class(h, _common_class((z, q_pre, cq, h)))
    _launch("gru_blend", (z, q_pre, cq, h, h_out), ("z", "q_pre", "cq", "h", "h_out"))
    return h_out


def gru_gates_backward(g_z, g_rh, z, r_pre, cr, h, g_zpre=None, g_rpre=None, g_h=None):
    """The gradients of ``gru_gates`` from those of its outputs, one launch
    (rc_gru_gates_backward): g_zpre = g_z * (1 - z) * z, g_rpre = g_rh * h *
    (1 - r) * r and g_h = g_rh * r, with r = sigmoid(r_pre + cr) recomputed.
    g_zpre and g_rpre are the gradients of cz and cr as well.  Operands as for
    ``gru_gates``; an output may be an input (``g_zpre`` over ``g_z``), the
    outputs are three different tensors and are allocated when missing.
    Returns (g_zpre, g_rpre, g_h)."""
    ins = (g_z, g_rh, z, r_pre, cr, h)
    cls = _common_class([t for t in ins if isinstance(t, torch.Tensor) and t.dim() == 4])
    outs = [_empty_like_class(h, cls) if t is None else t for t in (g_zpre, g_rpre, g_h)]
    _launch("gru_gates_backward", (*ins, *outs),
            ("g_z", "g_rh", "z", "r_pre", "cr", "h", "g_zpre", "g_rpre", "g_h"))
    return tuple(outs)


def gru_blend_backward(g_out, z, q_pre, cq, h, g_z=None, g_qpre=None, g_h=None):
    """The gradients of ``gru_blend`` from that of its output, one launch
    (rc_gru_blend_backward): g_z = g_out * (q - h), g_qpre = g_out * z *
    (1 - q*q) (the gradient of cq as well) and g_h = g_out * (1 - z), with
    q = tanh(q_pre + cq) recomputed.  Operands as for ``gru_gates``; an output
    may be an input (``g_h`` over ``g_out``), the outputs are three different
    tensors and are allocated when missing.  Returns (g_z, g_qpre, g_h)."""
    ins = (g_out, z, q_pre, cq, h)
    cls = _common_class([t for t in ins if isinstance(t, torch.Tensor) and t.dim() == 4])
    outs = [_empty_like_class(h, cls) if t is None else t for t in (g_z, g_qpre, g_h)]
    _launch("gru_blend_backward", (*ins, *outs), ("g_out", "z", "q_pre", "cq", "h", "g_z", "g_qpre", "g_h"))
    return tuple(outs)


def why_not_assemblable(parts, dtype, memory_format=torch.contiguous_format, out=None, differentiable=False):
    """None when ``assemble`` can fill the buffer from ``parts`` (tensors and
    ``Pooled`` / ``Resized`` descriptors), else the first reason why not, in
    words.  ``differentiable``: for ``assemble(differentiable=True)``, which a
    gradient being recorded does not stop (it cannot fill ``out`` then)."""
    parts = tuple(parts)
    if not 1 <= len(parts) <= _lib.RC_GRU_MAX_PARTS:
        return f"{len(parts)} parts: 1 to {_lib.RC_GRU_MAX_PARTS}"
    if any(not _is_part(t) or t.dim() != 4 for t in parts):
        return "parts that are not 4-D tensors or Pooled / Resized descriptors"
    if dtype not in _CODES:
        return f"dtype {dtype}: float32, float16 or bfloat16"
    if any(t.dtype not in _CODES for t in parts):
        return "a part that is not float32, float16 or bfloat16"
    first = parts[0]
    if any(t.shape[0] != first.shape[0] or t.shape[2:] != first.shape[2:] for t in parts):
        return "parts whose batch or spatial sizes differ"
    if any(t.shape[1] < 1 or min(_src(t).shape[2:]) < 1 for t in parts):
        return "an empty part"
    recorded = torch.is_grad_enabled() and any(t.requires_grad for t in parts)
    if recorded and not differentiable:
        return "a gradient is being recorded (the assembly has no backward)"
    if recorded and out is not None:
        return "a gradient is being recorded and out is given (autograd does not see a buffer filled in place)"
    if first.device.type != "cuda":
        return f"the parts are on {first.device}: HIP devices only"
    if any(t.device != first.device for t in parts):
        return "parts on different devices"
    if memory_format not in (torch.contiguous_format, torch.channels_last):
        return f"memory_format {memory_format}: contiguous_format or channels_last"
    if out is not None:
        want = (first.shape[0], sum(t.shape[1] for t in parts), *first.shape[2:])
        if not isinstance(out, torch.Tensor) or tuple(out.shape) != want or out.dtype != dtype \
                or out.device != first.device:
            return f"out is not a {dtype} tensor of shape {want} on the parts' device"
        if not _classes(out):
            return "out is neither planar nor interleaved"
        if any(_src(t).data_ptr() == out.data_ptr() for t in parts):
            return "out is one of the sources"
    return None


def _sources_fit(parts, cls):
    """Whether every part's source is of the buffer's layout class, so that
    ``assemble`` moves whole vectors.  It computes the same values from any
    strides, but then one element per lane, and with gru08's NCHW motion
    features in a channels_last network that lost end to end against
    ``interp`` + ``torch.cat`` (``e2e_bf16_cl_any`` in
    profiles/gru_inputs.json).  ``conv_gru_forward`` leaves such inputs to the
    PyTorch ops unless ``gru.fuse_inputs == "any"`` asks for the launch
    whatever the formats are (tools/e2e_probe.py measures with it)."""
    return all(_classes(_src(t)) & cls for t in parts)


def _src(t):
    return t.src if isinstance(t, _Lazy) else t


def assemble(parts, dtype, memory_format=torch.contiguous_format, out=None, differentiable=False):
    """The concatenation of ``parts`` along the channels as a ``dtype`` tensor
    of ``memory_format``, one launch (rc_gru_assemble) on the current stream:
    a tensor is copied (and cast), a ``Pooled`` / ``Resized`` descriptor is
    computed from its source straight into its channels.  ``out``: the buffer
    to fill (planar or interleaved; a channel slice of a larger one will do)
    instead of a new one.  Returns the buffer.  No CPU fallback.
    ``differentiable``: where a gradient is being recorded for a part, the
    result carries an autograd node whose backward is one launch of
    ``assemble_backward``; it saves no tensor (the adjoint is linear)."""
    parts = tuple(parts)
    for i, t in enumerate(parts):
        if _is_part(t) and t.device.type != "cuda":
            raise RuntimeError(f"assemble: part {i} is on {t.device}; the kernel runs on HIP devices only "
                               "(no CPU fallback)")
    why = why_not_assemblable(parts, dtype, memory_format, out, differentiable)
    if why is not None:
        raise ValueError(f"assemble: {why}")
    if differentiable and torch.is_grad_enabled() and any(t.requires_grad for t in parts):
        return _AssembleFn.apply(None, _kinds(parts), dtype, memory_format, *[_src(t) for t in parts])
    first = parts[0]
    N, _, H, W = first.shape
    if out is None:
        out = torch.empty((N, sum(t.shape[1] for t in parts), H, W), dtype=dtype, device=first.device,
                          memory_format=memory_format)
    srcs = [_src(t) for t in parts]
    modes = [_MODES[t.mode] if isinstance(t, _Lazy) else _lib.RC_PART_COPY for t in parts]
    n = len(parts)
    with torch.cuda.device(first.device):
        stream = torch.cuda.current_stream(first.device).cuda_stream or None
        rc = _lib.lib().rc_gru_assemble(
            out.data_ptr(), _lib.long_array(out.stride()), _CODES[dtype], N, H, W, n,
            _lib.ptr_array([t.data_ptr() for t in srcs]), _lib.long_array([v for t in srcs for v in t.stride()]),
            _lib.int_array([_CODES[t.dtype] for t in srcs]), _lib.int_array(modes),
            _lib.int_array([t.shape[1] for t in srcs]), _lib.int_array([t.shape[2] for t in srcs]),
            _lib.int_array([t.shape[3] for t in srcs]), stream)
    _lib.check(rc, "rc_gru_assemble")
    return out


def _parts_meta(parts):
    """What ``assemble_backward`` needs of each part: (mode, the source's
    shape, the source's dtype)."""
    return tuple((t.mode if isinstance(t, _Lazy) else "copy", tuple(_src(t).shape), t.dtype) for t in parts)


def assemble_backward(g, parts_meta, skip=(), g2=None, g2_from=0):
    """The gradients of the sources of ``assemble`` from the gradient ``g`` of
    its result, one launch (rc_gru_assemble_backward) on the current stream.
    ``parts_meta``: one (mode, source shape, source dtype) per part with mode
    "copy", "pool2x" or "bilinear" (``_parts_meta``); ``skip``: the indices of
    the parts whose gradient is not wanted (their channels still count).
    ``g2``: a second gradient of g's shape, strides and dtype; the channels
    from ``g2_from`` on use g + g2 (added in fp32).  g is planar or
    interleaved.  Returns one tensor per part, None for a skipped one, each
    in its source's dtype and g's memory format.  No CPU fallback."""
    parts_meta = tuple(parts_meta)
    for t, n in ((g, "g"), (g2, "g2")):
        if t is None and n == "g2":
            continue
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"assemble_backward: {n} must be a torch.Tensor")
        if t.device.type != "cuda":
            raise RuntimeError(f"assemble_backward: {n} is on {t.device}; the kernel runs on HIP devices only "
                               "(no CPU fallback)")
    if g.dim() != 4 or g.dtype not in _CODES:
        raise ValueError(f"assemble_backward: g of shape {tuple(g.shape)} and {g.dtype}: 4-D, float32, float16 or "
                         "bfloat16")
    if not 1 <= len(parts_meta) <= _lib.RC_GRU_MAX_PARTS:
        raise ValueError(f"assemble_backward: {len(parts_meta)} parts: 1 to {_lib.RC_GRU_MAX_PARTS}")
    if any(m not in _MODES or len(shape) != 4 or dt not in _CODES for m, shape, dt in parts_meta):
        raise ValueError("assemble_backward: parts_meta holds (mode, 4-D source shape, float dtype) entries")
    N, C, H, W = g.shape
    if C != sum(shape[1] for _, shape, _ in parts_meta) or any(shape[0] != N for _, shape, _ in parts_meta):
        raise ValueError(f"assemble_backward: g has shape {tuple(g.shape)}, the parts "
                         f"{[shape for _, shape, _ in parts_meta]}")
    if g2 is not None and (g2.shape != g.shape or g2.dtype != g.dtype or g2.device != g.device
                           or g2.stride() != g.stride()):
        raise ValueError("assemble_backward: g2 differs from g in shape, strides, dtype or device")
    cls = _classes(g)
    if not cls:
        raise ValueError(f"assemble_backward: g is neither planar nor interleaved (strides {g.stride()})")
    fmt = torch.contiguous_format if "planar" in cls else torch.channels_last
    skip = set(skip)
    outs = [None if i in skip else torch.empty(shape, dtype=dt, device=g.device, memory_format=fmt)
            for i, (_, shape, dt) in enumerate(parts_meta)]
    n = len(parts_meta)
    with torch.cuda.device(g.device):
        stream = torch.cuda.current_stream(g.device).cuda_stream or None
        rc = _lib.lib().rc_gru_assemble_backward(
            g.data_ptr(), None if g2 is None else g2.data_ptr(), int(g2_from), _lib.long_array(g.stride()),
            _CODES[g.dtype], N, H, W, n, _lib.ptr_array([None if t is None else t.data_ptr() for t in outs]),
            _lib.long_array([v for t in outs for v in ((0, 0, 0, 0) if t is None else t.stride())]),
            _lib.int_array([_CODES[dt] for _, _, dt in parts_meta]), _lib.int_array([_MODES[m] for m, _, _ in parts_meta]),
            _lib.int_array([shape[1] for _, shape, _ in parts_meta]),
            _lib.int_array([shape[2] for _, shape, _ in parts_meta]),
            _lib.int_array([shape[3] for _, shape, _ in parts_meta]), stream)
    _lib.check(rc, "rc_gru_assemble_backward")
    return outs


def _as_class(t, cls):
    """t itself when it fits a class of ``cls``, else a copy that does (a
    convolution that answered in another memory format than its input's)."""
    if _classes(t) & cls:
        return t
    return t.contiguous(memory_format=torch.contiguous_format if "planar" in cls else torch.channels_last)


def _one(cls):
    return {"planar"} if "planar" in cls else {"interleaved"}


class _GatesFn(torch.autograd.Function):
    """(zr, cz, cr, h) -> (z, r*h) on rc_gru_gates; zr is the stacked z/r
    convolution's output.  Saves z, the r_pre half of zr, cr and h; none of
    them is written after this."""

    @staticmethod
    def forward(ctx, zr, cz, cr, h):
        C = h.shape[1]
        r_pre = zr[:, C:]
        z, rh = gru_gates(zr[:, :C], r_pre, cz, cr, h)
        ctx.save_for_backward(z, r_pre, cr, h)
        return z, rh

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_z, g_rh):
        z, r_pre, cr, h = ctx.saved_tensors
        N, C, H, W = h.shape
        cls = _one(_common_class((z, r_pre, cr, h)))
        fmt = torch.contiguous_format if "planar" in cls else torch.channels_last
        g_zr = torch.empty((N, 2 * C, H, W), dtype=h.dtype, device=h.device, memory_format=fmt)
        g_zpre, g_rpre, g_h = gru_gates_backward(_as_class(g_z, cls), _as_class(g_rh, cls), z, r_pre, cr, h,
                                                 g_zpre=g_zr[:, :C], g_rpre=g_zr[:, C:])
        return g_zr, g_zpre, g_rpre, g_h


class _BlendFn(torch.autograd.Function):
    """(z, q_pre, cq, h) -> the new hidden state on rc_gru_blend; saves its
    four inputs."""

    @staticmethod
    def forward(ctx, z, q_pre, cq, h):
        ctx.save_for_backward(z, q_pre, cq, h)
        return gru_blend(z, q_pre, cq, h)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_out):
        z, q_pre, cq, h = ctx.saved_tensors
        cls = _one(_common_class((z, q_pre, cq, h)))
        g_z, g_qpre, g_h = gru_blend_backward(_as_class(g_out, cls), z, q_pre, cq, h)
        return g_z, g_qpre, g_qpre, g_h


class _Call:
    """What the two assembly nodes of one training call share: the gradient
    of [r*h, x] on its way from ``_TailFn.backward`` to ``_AssembleFn.backward``."""
    g_rx = None


def _kinds(parts):
    """The parts without their tensors: (mode, output size) each."""
    return tuple((t.mode, t.shape[2:]) if isinstance(t, _Lazy) else ("copy", None) for t in parts)


def _class_of(fmt):
    return {"planar"} if fmt == torch.contiguous_format else {"interleaved"}


class _AssembleFn(torch.autograd.Function):
    """(the parts' sources) -> the assembled buffer on rc_gru_assemble; the
    backward is one rc_gru_assemble_backward launch.  Saves no tensor: shapes,
    dtypes and modes only.  With a ``call`` (the training route of
    ``conv_gru_forward``) part 0 is h: its gradient is the first channels of
    the incoming one, and the gradient that ``_TailFn.backward`` left in
    ``call`` joins the other parts' inside the launch."""

    @staticmethod
    def forward(ctx, call, kinds, dtype, fmt, *sources):
        parts = [t if m == "copy" else (Pooled(t) if m == "pool2x" else Resized(t, size))
                 for t, (m, size) in zip(sources, kinds)]
        ctx.call, ctx.meta, ctx.fmt = call, _parts_meta(parts), fmt
        return assemble(parts, dtype, fmt)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        call, meta = ctx.call, ctx.meta
        g = _as_class(g, _class_of(ctx.fmt))
        g2, C = None, 0
        skip = {i for i in range(len(meta)) if not ctx.needs_input_grad[4 + i]}
        if call is not None:
            g2, call.g_rx = call.g_rx, None         # dropped after use: a second backward stores it again
            C = meta[0][1][1]
            skip.add(0)
            if g2 is not None and g2.stride() != g.stride():
                g, g2 = g.contiguous(memory_format=ctx.fmt), g2.contiguous(memory_format=ctx.fmt)
        outs = [None] * len(meta)
        if len(skip) < len(meta):
            outs = assemble_backward(g, meta, skip, g2=g2, g2_from=C)
        if call is not None and ctx.needs_input_grad[4]:
            outs[0] = g[:, :C]
        return (None, None, None, None, *outs)


class _TailFn(torch.autograd.Function):
    """(hx, rh) -> [r*h, x], the second buffer of the training route: one
    rc_gru_assemble launch with two copied parts, rh and hx's x channels.  Its
    backward hands rh its channels of the gradient and leaves the whole
    gradient in ``call`` for ``_AssembleFn.backward``, which runs later (rx
    depends on hx through the gate convolution as well) and adds the x
    channels to its own inside its launch; hx gets nothing from here."""

    @staticmethod
    def forward(ctx, call, fmt, hx, rh):
        ctx.call, ctx.fmt, ctx.C = call, fmt, rh.shape[1]
        return assemble((rh, hx[:, ctx.C:]), hx.dtype, fmt)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        g = _as_class(g, _class_of(ctx.fmt))
        ctx.call.g_rx = g
        return None, None, None, g[:, :ctx.C]


def _records_grad(gru, tensors):
    """Whether autograd would record a gradient for an input or a gate weight."""
    if not torch.is_grad_enabled():
        return False
    params = [p for c in (gru.convz, gru.convr, gru.convq) for p in (c.weight, c.bias) if p is not None]
    return any(t.requires_grad for t in tensors) or any(p.requires_grad for p in params)


def _conv_gru_train(gru, h, cz, cr, cq, x_list, cls):
    """The training route of ``conv_gru_forward``: every step an autograd
    node.  Each part is cast before the concatenation (``torch.cat(out=)``
    records no gradient), and [r*h, x] is a second buffer: the stacked
    convolution has saved [h, x].  With ``gru.fuse_inputs_backward`` set, and
    where ``assemble`` takes the parts and every source is of the buffer's
    layout class (``_sources_fit``, the rule of the inference route), the two
    buffers are one ``assemble`` launch each and their backward is one
    ``assemble_backward`` launch (``_AssembleFn``, ``_TailFn``): no pooled,
    resized or cast tensor, no concatenation and no accumulation add per part."""
    dt = h.dtype
    C = h.shape[1]
    one = _one(cls)
    fmt = torch.contiguous_format if "planar" in one else torch.channels_last
    call = None
    if getattr(gru, "fuse_inputs_backward", False) \
            and why_not_assemblable((h, *x_list), dt, fmt, differentiable=True) is None \
            and _sources_fit(x_list, one):
        call = _Call()
        hx = _AssembleFn.apply(call, _kinds((h, *x_list)), dt, fmt, h, *[_src(t) for t in x_list])
    else:
        xs = [x.to(dt) for x in materialized(x_list)]
        hx = torch.cat([h, *xs], dim=1).contiguous(memory_format=fmt)
    w, b, _ = _zr_conv(gru)
    zr = _as_class(F.conv2d(hx, w, b, padding=gru.convz.padding, dilation=gru.convz.dilation), one)
    z, rh = _GatesFn.apply(zr, cz, cr, h)
    if call is not None:
        rx = _TailFn.apply(call, fmt, hx, rh)
    else:
        rx = torch.cat([rh, *xs], dim=1).contiguous(memory_format=fmt)
    q = _as_class(gru.convq(rx), one)
    return _BlendFn.apply(z, q, cq, h)


def conv_gru_forward(gru, h, cz, cr, cq, *x_list, differentiable=False):
    """``ConvGRU.forward`` for arguments that are ``fusable``: the same three
    convolutions, one concatenation and two elementwise launches (module
    docstring).  Returns the new hidden state, a new tensor in h's layout.
    ``differentiable``: where a gradient is being recorded for an input or a
    gate weight, record a first-order autograd graph whose glue is the two
    backward kernels (arguments that are ``fusable(differentiable=True)``);
    with nothing to record this is the inference route.  ``Pooled`` /
    ``Resized`` parts of x: with ``gru.fuse_inputs`` set the inference route
    computes them inside the launch that fills the [h, x] buffer
    (``assemble``), and with ``gru.fuse_inputs_backward`` set so does the
    training route, whose backward is then one ``assemble_backward`` launch;
    otherwise they are materialised with the PyTorch ops before anything
    else."""
    cls = _common_class((h, cz, cr, cq))
    if not cls:
        raise ValueError("conv_gru_forward: h, cz, cr and cq share no layout class (see gru.fusable)")
    if differentiable and _records_grad(gru, (h, cz, cr, cq, *x_list)):
        return _conv_gru_train(gru, h, cz, cr, cq, x_list, cls)
    dt = h.dtype
    N, C, H, W = h.shape
    fmt = torch.contiguous_format if "planar" in cls else torch.channels_last
    lazy = getattr(gru, "fuse_inputs", False)
    if lazy and why_not_assemblable((h, *x_list), dt, fmt) is None \
            and (lazy == "any" or _sources_fit(x_list, _one(cls))):
        hx = assemble((h, *x_list), dt, fmt)            # pool2x, interp and the concatenation, one launch
    else:
        x_list = materialized(x_list)
        Cx = sum(x.shape[1] for x in x_list)
        hx = torch.empty((N, C + Cx, H, W), dtype=dt, device=h.device, memory_format=fmt)
        torch.cat([h, *x_list], dim=1, out=hx)
    one = _one(cls)
    w, b, _ = _zr_conv_as(gru, dt)
    zr = _as_class(F.conv2d(hx, w, b, padding=gru.convz.padding, dilation=gru.convz.dilation), one)
    z = zr[:, :C]
    gru_gates(z, zr[:, C:], cz, cr, h, z_out=z, rh_out=hx[:, :C])      # hx is now [r*h, x]
    q = _as_class(gru.convq(hx), one)
    return gru_blend(z, q, cq, h)
