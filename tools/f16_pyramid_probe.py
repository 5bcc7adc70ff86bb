"""The fp16 pyramid against the bf16 one at the KITTI config.

    python tools/f16_pyramid_probe.py [--batches 64,8] [--reps 5] [--parent-lib PATH]
                                      [--out profiles/f16_pyramid.json]

Times, interleaved and with device events (no profiler), per variant:
the build alone, one pair lookup (median launch of the 32) and the corr step
(build + 32 lookups, the bench's step):

  bf16         bf16 fmaps -> bf16 pyramid: the yardstick;
  bf16_parent  the same through another build of the library (--parent-lib:
               libraftcorr.so of the parent commit), so that the yardstick is
               the code from before the fp16 element type;
  f16          fp16 fmaps -> fp16 pyramid (pyramid_dtype=torch.float16);
  f16_legacy   fp16 fmaps without the option: two .float() casts, then the
               fp32-fmap bf16 build (what an fp16-autocast network gets today).

The run-to-run spread of the yardstick (max - min over the repetitions) is
recorded beside the medians: a difference below it is not distinguishable.
Also records the per-level normalised error (max|a - ref| / max|ref|) of the
bf16 and fp16 pyramids of one batch element against the fp64-accumulated C
oracle on the same (bf16- / fp16-rounded) fmaps.
"""
import argparse
import contextlib
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bench  # noqa: E402
from golden_util import norm_err  # noqa: E402
from oracle import coracle  # noqa: E402
from raft_stereo_amd import CorrBlock1D, _lib  # noqa: E402


@contextlib.contextmanager
def library(dll):
    """Route every C-ABI call to ``dll`` (None: the product library)."""
    prev, _lib._active = _lib._active, dll
    try:
        yield
    finally:
        _lib._active = prev


def inputs(B, D, H, W1, W2, iters, dev, seed=1):
    """randn fmaps (fp32) and bench.py's random field x = w1 - U[0, 64), one
    coords tensor per iteration -- drawn on the device."""
    g = torch.Generator(device=dev).manual_seed(seed)
    f1 = torch.randn(B, D, H, W1, generator=g, device=dev)
    f2 = torch.randn(B, D, H, W2, generator=g, device=dev)
    grid = bench.coords_grid(B, H, W1).to(dev)
    cs = []
    for _ in range(iters):
        c = grid.clone()
        c[:, 0] -= torch.rand(B, H, W1, generator=g, device=dev) * 64.0
        cs.append(c)
    return f1, f2, cs


def time_variant(mk, cs, t):
    e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    torch.cuda._sleep(5_000_000)            # no host gap inside the events
    e[0].record()
    blk = mk()
    e[1].record()
    torch.cuda.synchronize()
    t["build"].append(e[0].elapsed_time(e[1]) * 1e3)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(cs) + 1)]
    torch.cuda._sleep(5_000_000)
    ev[0].record()
    for k, c in enumerate(cs):
        blk(c)
        ev[k + 1].record()
    torch.cuda.synchronize()
    t["lookup"].append(statistics.median(ev[k].elapsed_time(ev[k + 1]) * 1e3 for k in range(len(cs))))
    del blk
    s0, s1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda._sleep(5_000_000)
    s0.record()
    for _k in range(3):
        blk = mk()
        for c in cs:
            blk(c)
        del blk
    s1.record()
    torch.cuda.synchronize()
    t["step"].append(s0.elapsed_time(s1) * 1e3 / 3)


def measure(B, cfg, reps, parent, dev):
    _, D, H, W1, W2, L, r, iters, _ = cfg
    f1, f2, cs = inputs(B, D, H, W1, W2, iters, dev)
    b1, b2, h1, h2 = f1.bfloat16(), f2.bfloat16(), f1.half(), f2.half()
    del f1, f2
    kw = dict(num_levels=L, radius=r)
    variants = {
        "bf16": (None, lambda: CorrBlock1D(b1, b2, **kw)),
        "f16": (None, lambda: CorrBlock1D(h1, h2, pyramid_dtype=torch.float16, **kw)),
        "f16_legacy": (None, lambda: CorrBlock1D(h1, h2, **kw)),
    }
    if parent is not None:
        variants["bf16_parent"] = (parent, variants["bf16"][1])
    res = {"B": B}
    with torch.no_grad():
        # the two pyramids serve the same lookups: fp16 is read by the pair kernel's fp16 twin
        x, y = variants["bf16"][1](), variants["f16"][1]()
        assert x.pyramid_dtype == torch.bfloat16 and y.pyramid_dtype == torch.float16
        assert x._chain and y._chain and x.levels_stored == y.levels_stored and x._shadow == y._shadow
        res["levels_stored"], res["shadow"] = list(x.levels_stored), sorted(x._shadow)
        res["max_abs_diff_f16_vs_bf16_lookup"] = float((x(cs[0]) - y(cs[0])).abs().max())
        del x, y
        t = {v: {"build": [], "lookup": [], "step": []} for v in variants}
        for v, (dll, mk) in variants.items():   # warm-up: code objects, allocator
            with library(dll):
                blk = mk()
                blk(cs[0])
                del blk
        for _ in range(reps):
            for v, (dll, mk) in variants.items():
                with library(dll):
                    time_variant(mk, cs, t[v])
    res["us"] = {v: {k: statistics.median(x) for k, x in d.items()} for v, d in t.items()}
    res["us_all"] = t
    yard = "bf16_parent" if parent is not None else "bf16"
    res["yardstick"] = yard
    res["spread_us"] = {k: max(x) - min(x) for k, x in t[yard].items()}
    res["f16_minus_yardstick_us"] = {k: res["us"]["f16"][k] - res["us"][yard][k] for k in ("build", "lookup", "step")}
    res["within_spread"] = {k: res["f16_minus_yardstick_us"][k] <= res["spread_us"][k]
                            for k in ("build", "lookup", "step")}
    return res


def errors(cfg, dev):
    """Per-level normalised error of one batch element's pyramids against the
    fp64-accumulated oracle on the same rounded fmaps."""
    _, D, H, W1, W2, L, r, iters, _ = cfg
    f1, f2, _cs = inputs(1, D, H, W1, W2, 0, dev, seed=2)
    out = {}
    with torch.no_grad():
        for name, dt in (("bf16", torch.bfloat16), ("f16", torch.float16)):
            a, b = f1.to(dt), f2.to(dt)
            blk = CorrBlock1D(a, b, num_levels=L, radius=r, pyramid_dtype=dt)
            got = [t.reshape(t.shape[0], -1).float().cpu().numpy() for t in blk.corr_pyramid]
            ref = coracle.corr_pyramid(a.float().cpu().numpy(), b.float().cpu().numpy(), L)
            out[name] = [norm_err(g, np.asarray(q)) for g, q in zip(got, ref)]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="kitti")
    ap.add_argument("--batches", default="64,8")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent-lib", default=None, help="libraftcorr.so built from the parent commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "f16_pyramid.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("f16_pyramid_probe: needs a HIP device (nothing is measured on the CPU)")
    dev = torch.device("cuda", 0)
    cfg = bench.CONFIGS[a.config]
    parent = _lib._open(a.parent_lib) if a.parent_lib else None
    res = {"config": a.config, "shape": dict(zip(("D", "H", "W1", "W2", "levels", "radius", "lookups"), cfg[1:8])),
           "reps": a.reps, "device": torch.cuda.get_device_name(0),
           "timing": "device events, interleaved repetitions; us; medians, spread = max - min of the yardstick",
           "runs": [measure(int(b), cfg, a.reps, parent, dev) for b in a.batches.split(",")],
           "norm_err_vs_fp64_oracle": errors(cfg, dev)}
    text = json.dumps(res, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text + "\n")
    brief = {k: v for k, v in res.items() if k != "runs"}
    brief["runs"] = [{k: v for k, v in r.items() if k != "us_all"} for r in res["runs"]]
    print(json.dumps(brief), flush=True)


if __name__ == "__main__":
    main()
