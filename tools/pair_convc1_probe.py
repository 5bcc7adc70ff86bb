"""Fused lookup + convc1: the pair-layout kernel against the per-level one and
against the unfused path (dev probe).

    python tools/pair_convc1_probe.py [--config 2|3] [--reps 9] [--calls 8] [--out FILE]

Four ways to get ``relu(convc1(lookup(coords)))`` on one block, timed in one
process, alternated, between device events (``calls`` launches at different
coords per sample, ``reps`` samples each, every path warmed first):

  per_level   rc_corr_lookup_conv on the full pyramid (every level in memory);
  pair_fp32   rc_corr_lookup_chain_conv on the stored levels 0 and 2, fp32 out;
  pair_fp16   the same with an fp16 output (RC_OUT_F16);
  unfused     the pair lookup, then the 1x1 conv (MIOpen) and ReLU.

Per path: the median per call in us, the min and max of the samples, and the
spread of the medians of ``--runs`` repeated identical runs.  Also the bytes
the block holds before and after its first fused call, the bytes the
per-level route would pool into it (levels 1, 3 and the top level), and
whether pair_fp32 equals per_level bit for bit.
config 2: fmaps 8 x 256 x 135 x 240, fp32 pyramid; config 3 (one GPU's share):
8 x 256 x 94 x 311 (375 x 1242 images at 1/4), bf16 pyramid.  Needs a HIP
device."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pkgload  # noqa: E402

pkgload.load()
from raft_stereo_amd import CorrBlock1D  # noqa: E402
from raft_stereo_amd import corr as rcorr  # noqa: E402

CONFIGS = {2: ((8, 256, 135, 240), torch.float32), 3: ((8, 256, 94, 311), torch.bfloat16)}


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=2, choices=sorted(CONFIGS))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--calls", type=int, default=8)
    ap.add_argument("--cout", type=int, default=64)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("pair_convc1_probe: needs a HIP device")
    (B, D, H, W), pd = CONFIGS[a.config]
    L, r, cout = 4, 4, a.cout
    cin = L * (2 * r + 1)
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(11)
    fd = torch.bfloat16 if pd == torch.bfloat16 else torch.float32
    f1 = torch.randn(B, D, H, W, generator=g).to(dev).to(fd)
    f2 = torch.randn(B, D, H, W, generator=g).to(dev).to(fd)
    wgt = (torch.randn(cout, cin, 1, 1, generator=g) / cin ** 0.5).to(dev)
    bias = (torch.randn(cout, generator=g) * 0.1).to(dev)
    base = torch.arange(W).float().view(1, 1, 1, W) - torch.rand(B, 1, H, W, generator=g) * 32
    coords = [torch.cat([base + 0.37 * i, torch.zeros_like(base)], 1).to(dev) for i in range(a.calls)]
    res = {"config": a.config, "fmaps": [B, D, H, W], "pyramid": str(pd), "cout": cout, "calls": a.calls,
           "reps": a.reps, "runs": a.runs}
    with torch.no_grad():
        torch.cuda.synchronize()
        m0 = torch.cuda.memory_allocated()
        blk = CorrBlock1D(f1, f2, num_levels=L, radius=r, pyramid_dtype=pd)
        torch.cuda.synchronize()
        m1 = torch.cuda.memory_allocated()
        out = blk.lookup_convc1(coords[0], wgt, bias)
        del out
        torch.cuda.synchronize()
        m2 = torch.cuda.memory_allocated()
        res["block_MB"] = round((m1 - m0) / 1e6, 1)
        res["block_after_fused_call_MB"] = round((m2 - m0) / 1e6, 1)
        res["levels_stored_after_fused_call"] = blk.levels_stored
        full = CorrBlock1D(f1, f2, num_levels=L, radius=r, pyramid_dtype=pd, lazy_levels=False)
        torch.cuda.synchronize()
        res["full_pyramid_block_MB"] = round((torch.cuda.memory_allocated() - m2) / 1e6, 1)
        pyr = full.corr_pyramid
        paths = {
            "per_level": lambda c: rcorr.lookup_convc1(pyr, c, L, r, wgt, bias, True),
            "pair_fp32": lambda c: blk.lookup_convc1(c, wgt, bias),
            "pair_fp16": lambda c: blk.lookup_convc1(c, wgt, bias, out_dtype=torch.float16),
            "unfused": lambda c: torch.relu(F.conv2d(blk(c), wgt, bias)),
        }
        x, y = paths["pair_fp32"](coords[0]), paths["per_level"](coords[0])
        res["pair_fp32_equals_per_level"] = bool(torch.equal(x.view(torch.int32), y.view(torch.int32)))
        res["pair_fp16_equals_cast"] = bool(torch.equal(paths["pair_fp16"](coords[0]).view(torch.int16),
                                                        y.half().view(torch.int16)))
        del x, y
        for fn in paths.values():                        # warm every path
            for c in coords:
                fn(c)
        torch.cuda.synchronize()
        medians = {name: [] for name in paths}
        samples = {name: [] for name in paths}
        for _ in range(a.runs):
            times = {name: [] for name in paths}
            for _ in range(a.reps):
                for name, fn in paths.items():           # alternate the paths
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda._sleep(2_000_000)         # let the host queue every launch first
                    e0.record()
                    for c in coords:
                        fn(c)
                    e1.record()
                    torch.cuda.synchronize()
                    times[name].append(e0.elapsed_time(e1) * 1e3 / len(coords))
            for name in paths:
                medians[name].append(median(times[name]))
                samples[name].extend(times[name])
        for name in paths:
            res[name] = {"median_us": round(median(samples[name]), 2),
                         "min_us": round(min(samples[name]), 2), "max_us": round(max(samples[name]), 2),
                         "run_medians_us": [round(m, 2) for m in medians[name]]}
        # what the per-level route would add to this block: levels 1, 3 and the top level pooled
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        blk._read_levels()
        torch.cuda.synchronize()
        res["per_level_route_pools_MB"] = round((torch.cuda.memory_allocated() - before) / 1e6, 1)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
