"""Guarded arena and raw C-ABI callers for the volume sweeps
(test_volume_sweep_gpu.py, test_volume_sweep_host.py) and, through
lookup_sweep_util.py, the lookup sweeps.

``arena`` carves every operand and output of one kernel call out of a single
buffer filled with a NaN bit pattern, at 16-byte-aligned addresses that are
deliberately not 128-byte aligned (two sub-line phases, 16 and 80 mod 128),
with at least 4 KiB of the pattern before and after each region.  After the
call ``assert_guards_intact`` compares the whole buffer with what it held
before the call, on an integer view: every byte outside the output regions --
the guard zones and the inputs -- must be bit-identical.  An over-read that
reaches the arithmetic meets NaN, so the callers also assert finite outputs.

The kernels are called through the C ABI with raw pointers (as
tests/test_capi.py does), so the addresses are the arena's and not an
allocator's.
"""
import numpy as np
import torch

from raft_stereo_amd import _lib

SENT32 = 0x7FC0DEAD          # a quiet fp32 NaN
SENT16 = 0x7FC1              # a quiet bf16 NaN; 0x7FC17FC1 is an fp32 NaN too
GUARD = 4096                 # bytes of sentinel before and after every region
PHASES = (16, 80)            # region address mod 128


def plan(sizes, base, phase=0):
    """Byte offsets of regions of ``sizes`` bytes in a buffer at address
    ``base``: region i at an address = PHASES[(phase + i) % 2] mod 128, GUARD
    bytes or more after the end of region i - 1 (or the buffer's start).
    Returns (offsets, total bytes incl. the trailing guard)."""
    offs, cur = [], GUARD
    for i, n in enumerate(sizes):
        want = PHASES[(phase + i) % 2]
        off = cur + (want - (base + cur)) % 128
        offs.append(off)
        cur = off + n + GUARD
    return offs, -(-cur // 4) * 4


def bound(sizes):
    """Bytes that hold ``plan(sizes, base, phase)`` for any base and phase."""
    return sum(n + GUARD + 128 for n in sizes) + GUARD + 4


class Arena:
    """specs: list of (name, nbytes, data) -- data a contiguous CPU tensor of
    nbytes bytes for an input, None for an output region -- or of (name,
    nbytes, data, True) for an in/out region: initial data that the call may
    change (an accumulating gradient buffer, coords updated in place)."""

    def __init__(self, dev, specs, phase=0, bf16=False):
        self.sent = (SENT16 << 16 | SENT16) if bf16 else SENT32
        specs = [(*s, False)[:4] for s in specs]
        sizes = [s[1] for s in specs]
        self.buf = torch.empty((bound(sizes) // 4 + 1,), dtype=torch.int32, device=dev)
        self.base = self.buf.data_ptr()
        offs, self.total = plan(sizes, self.base, phase)
        assert self.total <= self.buf.numel() * 4
        self.off, self.size, self.outputs = {}, {}, []
        image = torch.full((self.buf.numel(),), self.sent, dtype=torch.int32)
        u8 = image.view(torch.uint8)
        for (name, n, data, inout), off in zip(specs, offs):
            self.off[name], self.size[name] = off, n
            assert data is not None or not inout, name
            if data is None or inout:
                self.outputs.append(name)
            if data is not None:
                src = data.contiguous().reshape(-1).view(torch.uint8)
                assert src.numel() == n, (name, src.numel(), n)
                u8[off:off + n].copy_(src)
        self.buf.copy_(image)
        self.before = image.numpy().view(np.uint8)
        self.after = None

    def ptr(self, name):
        return self.base + self.off[name]

    def tensor(self, name, dtype, shape):
        """The region as a tensor view of the arena (no copy)."""
        es = torch.tensor([], dtype=dtype).element_size()
        o, n = self.off[name] // es, self.size[name] // es
        return self.buf.view(dtype)[o:o + n].view(shape)

    def fetch(self):
        self.after = self.buf.cpu().numpy().view(np.uint8)
        return self.after

    def region(self, name, np_dtype):
        a = self.after if self.after is not None else self.fetch()
        return a[self.off[name]:self.off[name] + self.size[name]].view(np_dtype)

    def assert_guards_intact(self):
        """Guards and inputs are bit-identical to their state before the
        call: only the output regions may differ."""
        a = self.fetch()
        keep = np.ones(a.size, bool)
        for name in self.outputs:
            keep[self.off[name]:self.off[name] + self.size[name]] = False
        bad = np.flatnonzero(keep & (a != self.before))
        if bad.size:
            b = int(bad[0])
            near = min(self.off, key=lambda k: min(abs(b - self.off[k]), abs(b - self.off[k] - self.size[k])))
            where = "before" if b < self.off[near] else "after the end of"
            dist = self.off[near] - b if b < self.off[near] else b - self.off[near] - self.size[near]
            inside = [k for k in self.off if self.off[k] <= b < self.off[k] + self.size[k]]
            msg = (f"input {inside[0]} modified at byte {b - self.off[inside[0]]}" if inside else
                   f"guard overwritten {dist} bytes {where} {near}")
            raise AssertionError(f"{msg} ({bad.size} bytes differ)")

    def assert_outputs_written(self, names, es=4):
        """No element (of es bytes) of the output regions ``names`` still
        holds the sentinel: the comparisons treat NaN == NaN, so an element
        the kernel never wrote would pass wherever the reference is NaN.  (No
        kernel produces the sentinel's payload: the hardware's own NaNs are
        0x7FC00000 / 0x7FC0 / 0x7E00, and a propagated input NaN would have to
        come from the poisoned padding, which must not be read.)"""
        for name in names:
            assert name in self.outputs, f"{name} is not an output region"
            if es == 2:
                left = np.flatnonzero(self.region(name, np.uint16) == SENT16)
            else:
                left = np.flatnonzero(self.region(name, np.uint32) == np.uint32(self.sent))
            assert not left.size, (f"output {name}: {left.size} of {self.size[name] // es} elements never "
                                   f"written, the first at index {int(left[0])}")


def arena(dev, specs, phase=0, bf16=False):
    return Arena(dev, specs, phase, bf16)


def bf16_to_f32(u16):
    return (u16.astype(np.uint32) << 16).view(np.float32)


def bf16_pool_np(level):
    """avg_pool2d([1,2]) of a bf16 level in fp32, rounded to bf16 (RNE), as
    PyTorch computes it on bf16 tensors."""
    t = torch.from_numpy(np.ascontiguousarray(level)).bfloat16().float()
    Wo = t.shape[1] // 2
    pm = (t[:, 0:2 * Wo:2] + t[:, 1:2 * Wo:2]) * 0.5
    return pm.bfloat16().float().numpy()


def f16_pool_np(level):
    """One pooling step of an fp16 level (given widened to fp32): the mean in
    fp32, rounded to fp16 (nearest even), widened again."""
    lv = np.asarray(level, np.float32)
    Wo = lv.shape[1] // 2
    with np.errstate(invalid="ignore", over="ignore"):
        pm = (lv[:, 0:2 * Wo:2] + lv[:, 1:2 * Wo:2]) * np.float32(0.5)
        return pm.astype(np.float16).astype(np.float32)


def integer_sweep(W2):
    """Every integer x from -40 to W2 + 40 with both fp32 neighbours."""
    k = np.arange(-40, W2 + 41, dtype=np.float32)
    return np.concatenate([k, np.nextafter(k, np.float32(np.inf)), np.nextafter(k, np.float32(-np.inf))])


def _es(dt):
    return 2 if dt == torch.bfloat16 else 4


def _code(dt):
    return _lib.RC_BF16 if dt == torch.bfloat16 else _lib.RC_F32


def level_ld(W, dt, pad):
    """Row stride (elements): dense, or rows padded to 16 bytes as
    CorrBlock1D stores them."""
    per16 = 16 // _es(dt)
    return -(-W // per16) * per16 if pad else W


def guarded_build(dev, f1, f2, pyr_dt, nbuf, stored=None, pad=False, flags=0, phase=0):
    """rc_corr_build on arena memory.  f1, f2: CPU tensors (B, D, H, W) fp32
    or bf16.  stored: the levels given a buffer (default all).  Returns the
    stored levels as fp32 arrays (P, W_l), None for the others; guards and
    inputs checked, outputs finite."""
    B, D, H, W1 = f1.shape
    W2 = f2.shape[3]
    P = B * H * W1
    stored = range(nbuf) if stored is None else stored
    es = _es(pyr_dt)
    lds = [level_ld(W2 >> l, pyr_dt, pad) for l in range(nbuf)]
    specs = [("f1", f1.numel() * f1.element_size(), f1), ("f2", f2.numel() * f2.element_size(), f2)]
    specs += [(f"l{l}", P * lds[l] * es, None) for l in stored]
    bf = torch.bfloat16 in (f1.dtype, pyr_dt)
    ar = arena(dev, specs, phase, bf)
    rc = _lib.lib().rc_corr_build(
        ar.ptr("f1"), ar.ptr("f2"), _code(f1.dtype), B, D, H, W1, W2,
        _lib.ptr_array([ar.ptr(f"l{l}") if l in stored else None for l in range(nbuf)]),
        _lib.long_array(lds) if pad else None, nbuf, _code(pyr_dt) | flags, None)
    _lib.check(rc, "rc_corr_build")
    ar.assert_guards_intact()
    out = []
    for l in range(nbuf):
        if l not in stored:
            out.append(None)
            continue
        raw = ar.region(f"l{l}", np.uint16 if es == 2 else np.float32)
        lvl = (bf16_to_f32(raw) if es == 2 else raw).reshape(P, lds[l])[:, :W2 >> l].copy()
        assert np.isfinite(lvl).all(), f"level {l}: non-finite output"
        out.append(lvl)
    return out


def guarded_records(dev, f1, f2, phase=0):
    """rc_corr_build with RC_LAYOUT_RECORDS on arena memory: (arena, the
    record tensor (P, NR, 64) bf16 as a view of it)."""
    B, D, H, W1 = f1.shape
    W2 = f2.shape[3]
    P, NR = B * H * W1, _lib.rec_count(W2)
    specs = [("f1", f1.numel() * 2, f1), ("f2", f2.numel() * 2, f2), ("rec", P * NR * _lib.RC_REC_BYTES, None)]
    ar = arena(dev, specs, phase, True)
    rc = _lib.lib().rc_corr_build(
        ar.ptr("f1"), ar.ptr("f2"), _lib.RC_BF16, B, D, H, W1, W2,
        _lib.ptr_array([ar.ptr("rec"), None, None]), _lib.long_array([W2, W2 >> 1, W2 >> 2]), 3,
        _lib.RC_BF16 | _lib.RC_LAYOUT_RECORDS, None)
    _lib.check(rc, "rc_corr_build")
    ar.assert_guards_intact()
    rec = ar.tensor("rec", torch.bfloat16, (P, NR, _lib.RC_REC_SLOTS))
    assert bool(torch.isfinite(rec.float()).all()), "records: non-finite slot"
    return ar, rec


def guarded_sheared(dev, f1, f2, num_levels, phase=0):
    """rc_corr_build with RC_LAYOUT_DISPARITY on arena memory: (arena,
    {level: flat fp32 tensor view}) as corr.build_sheared returns."""
    B, D, H, W1 = f1.shape
    W2 = f2.shape[3]
    ld = -(-W1 // 4) * 4
    keep = (0, 2) if num_levels == 4 else (0,)
    n = {l: B * H * _lib.shear_rows(W2, W1, l) * ld for l in keep}
    specs = [("f1", f1.numel() * 4, f1), ("f2", f2.numel() * 4, f2)] + [(f"s{l}", n[l] * 4, None) for l in keep]
    ar = arena(dev, specs, phase)
    nbuf = 3 if num_levels == 4 else 1
    ptrs = [ar.ptr(f"s{l}") if l in keep else None for l in range(nbuf)]
    rc = _lib.lib().rc_corr_build(
        ar.ptr("f1"), ar.ptr("f2"), _lib.RC_F32, B, D, H, W1, W2, _lib.ptr_array(ptrs),
        _lib.long_array([ld, W2 >> 1, ld][:nbuf]), nbuf, _lib.RC_F32 | _lib.RC_LAYOUT_DISPARITY, None)
    _lib.check(rc, "rc_corr_build")
    ar.assert_guards_intact()
    return ar, {l: ar.tensor(f"s{l}", torch.float32, (n[l],)) for l in keep}


def grad_ld(W):
    return -(-W // 4) * 4


def guarded_build_backward(dev, f1, f2, grads, exact=False, phase=0):
    """rc_corr_build_backward on arena memory.  grads: per level a CPU fp32
    tensor (P, grad_ld(W_l)) (zero row padding, as corr.grad_buffers keeps
    it) or None (a folded level of the pair layout).  Returns (df1, df2)."""
    B, D, H, W1 = f1.shape
    W2 = f2.shape[3]
    specs = [("f1", f1.numel() * 4, f1), ("f2", f2.numel() * 4, f2)]
    specs += [(f"g{l}", g.numel() * 4, g) for l, g in enumerate(grads) if g is not None]
    specs += [("df1", f1.numel() * 4, None), ("df2", f2.numel() * 4, None)]
    ar = arena(dev, specs, phase)
    rc = _lib.lib().rc_corr_build_backward(
        ar.ptr("f1"), ar.ptr("f2"), _lib.RC_F32 | (_lib.RC_BUILD_EXACT_F32 if exact else 0), B, D, H, W1, W2,
        _lib.ptr_array([None if g is None else ar.ptr(f"g{l}") for l, g in enumerate(grads)]),
        _lib.long_array([W2 >> l if g is None else g.shape[1] for l, g in enumerate(grads)]),
        len(grads), ar.ptr("df1"), ar.ptr("df2"), None)
    _lib.check(rc, "rc_corr_build_backward")
    ar.assert_guards_intact()
    df1 = ar.region("df1", np.float32).reshape(f1.shape).copy()
    df2 = ar.region("df2", np.float32).reshape(f2.shape).copy()
    assert np.isfinite(df1).all() and np.isfinite(df2).all(), "non-finite gradient"
    return df1, df2


# --------------------------------------------------------------- geometry
# Python restatements of the two dispatch rules, for the coverage assertions
# of test_volume_sweep_host.py and the table in test_volume_sweep_gpu.py.

def tile_frags(W):
    """csrc/volume_split.hip, rc_launch_build_split: a row of nf 16-column
    fragments goes in ceil(nf / 8) tiles of equal size."""
    nf = (W + 15) // 16
    nt = (nf + 7) // 8
    return (nf + nt - 1) // nt


def split_tile_frags(W):
    """Fragment count of every tile of a row of width W, the last partial
    one included (build_split_kernel switches on these at run time)."""
    nf, tf = (W + 15) // 16, tile_frags(W)
    return [min(tf, nf - t) for t in range(0, nf, tf)]


def split_pairs(W1, W2):
    """The (fa, fb) fragment-count pairs of the tiles of a (W1, W2) build."""
    return {(fa, fb) for fa in split_tile_frags(W1) for fb in split_tile_frags(W2)}


B16_PLAIN = [(4, 5), (4, 4), (3, 5), (3, 4), (2, 5), (2, 4)]      # cand[], in its order
B16_DEFER = [(5, 4), (4, 4), (3, 4), (2, 4)]                      # cand_defer[]
B16_BK = 32                                                       # kB16BK


def bf16_ring_shape(W2, D, defer):
    """csrc/volume.hip, bf16_ring_shape: (nwn, fma) with the fewest padded w2
    columns, the first candidate on ties; None = the per-wave kernel.  (The
    1 GiB image limit and the levels past kB16MaxFused do not bind at the
    sweeps' sizes.)"""
    if W2 <= 64 or (D + B16_BK - 1) // B16_BK < 2:
        return None
    best, bestpad = None, 0
    for nwn, fma in (B16_DEFER if defer else B16_PLAIN):
        w = 16 * fma * nwn
        pad = (W2 + w - 1) // w * w
        if best is None or pad < bestpad:
            best, bestpad = (nwn, fma), pad
    return best


def ranges(vals):
    """Sorted ints -> 'a-b, c-d' text."""
    out, vals = [], sorted(vals)
    i = 0
    while i < len(vals):
        j = i
        while j + 1 < len(vals) and vals[j + 1] == vals[j] + 1:
            j += 1
        out.append(f"{vals[i]}-{vals[j]}" if j > i else f"{vals[i]}")
        i = j + 1
    return ", ".join(out)


# ------------------------------------------------------------ sweep lists
# Shared by the GPU sweeps and the host-side coverage assertions.

def bands(vals, n):
    vals = list(vals)
    return [vals[i:i + n] for i in range(0, len(vals), n)]


M4 = list(range(4, 133, 4))                         # 4, 8, .., 132

# part 2: bf16 builds (B = 1, D = 72 unless given)
BF16_D = 72
BF16_W2 = list(range(65, 401))                      # at W1 = 24, forms a, b, c
BF16_W2_BANDS = bands(BF16_W2, 48)
BF16_W2_WIDE = list(range(481, 513, 8)) + [512] + list(range(721, 769, 8)) + [768]   # form b
BF16_W1 = list(range(1, 261))                       # at W2 = 70 and 311, forms a, b
BF16_W1_BANDS = bands(BF16_W1, 52)
BF16_W1_W2 = [70, 311]
BF16_DS = [33, 40, 63, 64, 65, 96, 97, 128, 160, 225, 256, 264]
BF16_D_PLAIN_W2 = [100, 150, 180, 230, 250, 311]
BF16_D_DEFER_W2 = [100, 150, 230, 311]
# the per-wave kernel: one 32-d stage at W2 = 100, and W2 <= 64; aligned
# (W1, W2 multiples of 8) and unaligned forms.  (D, W1, W2)
BF16_PERWAVE = ([(D, W1, 100) for D in (1, 8, 31, 32) for W1 in (40, 37)] +
                [(D, W1, W2) for D in (8, 40, 72) for W1 in (40, 37) for W2 in (8, 16, 33, 48, 53, 64)])
F32IN_D = 40
F32IN_W2 = list(range(2, 141))                      # at W1 = 20
F32IN_W1 = list(range(1, 141))                      # at W2 = 36
REC_W2 = list(range(65, 321))
REC_W2_BANDS = bands(REC_W2, 32)
REC_W1 = [8, 70]
REC_D = [225, 256]

# part 3: fp32 builds (B = 1, H = 1, D = 40 unless given)
F32_D = 40
SPLIT_CROSS_BANDS = bands(M4, 3)                    # W1 bands; every W2 of M4 in each
BAL_W = list(range(132, 257, 4))
BAL_PARTNERS = [16, 44, 100, 128, 240]
BAL_EXTRA = [272, 720]                              # three and six tiles
BAL_SHAPES = ([(w, p) for w in BAL_W + BAL_EXTRA for p in BAL_PARTNERS] +
              [(p, w) for w in BAL_W + BAL_EXTRA for p in BAL_PARTNERS])
SPLIT_DS = [1, 3, 4, 15, 16, 17, 31, 32, 33, 40, 48, 64, 96, 128, 256]
SPLIT_D_SHAPES = [(20, 36), (132, 72)]
RING3_DS = [17, 33, 48]                             # at (16, 16), H over two workgroups per CU
EXACT_W2 = list(range(1, 141))                      # at W1 = 21
EXACT_W1 = list(range(1, 141))                      # at W2 = 37
EXACT_VEC_W = list(range(4, 145, 4))
EXACT_VEC_PARTNERS = [4, 60, 128, 132]
EXACT_VEC_SHAPES = ([(w, p) for w in EXACT_VEC_W for p in EXACT_VEC_PARTNERS] +
                    [(p, w) for w in EXACT_VEC_W for p in EXACT_VEC_PARTNERS])
DISP_PARTNERS = [16, 44, 100, 132]
DISP_SHAPES = [(w, p) for w in M4 for p in DISP_PARTNERS] + [(p, w) for w in M4 for p in DISP_PARTNERS]

# part 4: volume backward (B = 1, D = 40 unless given)
BWD_D = 40
BWD_PARTNERS = [4, 36, 64, 100, 132]
BWD_LAYOUTS = ["pair4", "pair2", "level2"]
BWD_SHAPES = sorted(set([(w, p) for w in M4 for p in BWD_PARTNERS] + [(p, w) for w in M4 for p in BWD_PARTNERS]))
BWD_EXACT_W2 = list(range(1, 141))                  # at W1 = 21
BWD_EXACT_W1 = list(range(1, 141))                  # at W2 = 37
BWD_DS = [1, 3, 8, 15, 16, 17, 31, 32, 33, 40, 63, 64, 65, 100, 128, 129, 256]
BWD_D_SHAPES = [(36, 40), (132, 96), (311, 311)]    # the last: exact path only (W % 4 != 0)


def bwd_layout_ok(layout, W2):
    """pair4 folds a level 3 of width W2 >> 3 >= 1 into level 2; level2 needs
    a level 1 (capi.cpp, rc_corr_build_backward: `(W2 >> (levels - 1)) < 1`
    is RC_EINVAL)."""
    return W2 >= {"pair4": 8, "pair2": 4, "level2": 4}[layout]


def max_nbuf(W2, cap):
    """Largest nbuf <= cap rc_corr_build accepts (capi.cpp: `(W2 >> (nbuf -
    1)) < 1` is RC_EINVAL: pyramid level of width 0)."""
    return min(cap, W2.bit_length())
