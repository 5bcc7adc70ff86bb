"""A/B/C of the lookup output dtype: per case, interleaved
in one process,
  (a) the fp32 lookup,
  (b) the fp32 lookup followed by .to(dtype) -- what a mixed-precision
      network runs without the option (convc1's autocast cast),
  (c) the lookup that writes the dtype itself (CorrBlock1D(out_dtype=...)).

    python tools/outdtype_probe.py [--repeats 7] [--out profiles/outdtype_probe.json]
                                   [--kitti-batch 64] [--cases kitti,sceneflow]

Cases: config 3 (kitti, bf16 pyramid as records, B = 64) and config 2
(sceneflow, fp32 pyramid, the pair kernel), each NCHW and channels-last, for
fp16 and bf16.  Each repeat times every path once over the config's coords
(device events around all lookups of the pass, per-lookup mean); the JSON
holds, per case and path, the median over the repeats, their min and max
(the run-to-run spread) and the repeats themselves, after a bit-identity
check of (c) against (b).
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from raft_stereo_amd import CorrBlock1D, _lib  # noqa: E402


def time_pass(fn, coords):
    """Mean device time (us) of fn(c) over the coords, one event pair around
    the whole pass (a device sleep first: no host gap inside the events)."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda._sleep(5_000_000)
    e0.record()
    for c in coords:
        fn(c)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / len(coords)


def run_case(name, cfg, inputs, layout, cl, dtype, repeats):
    B, D, H, W1, W2, L, r, iters, _ = cfg
    f1, f2, cs = inputs
    kw = dict(num_levels=L, radius=r, channels_last=cl, layout=layout)
    blk = CorrBlock1D(f1, f2, **kw)             # one pyramid; out_dtype is read at call time

    def lookup(c, od):
        blk.out_dtype = od
        return blk(c)

    paths = {"a_fp32": lambda c: lookup(c, None), "b_fp32_then_cast": lambda c: lookup(c, None).to(dtype),
             "c_half_out": lambda c: lookup(c, dtype)}
    for c in cs[:2]:
        x, y = paths["b_fp32_then_cast"](c), paths["c_half_out"](c)
        assert y.dtype == dtype and torch.equal(torch.isnan(x), torch.isnan(y))
        assert torch.equal(torch.nan_to_num(x).contiguous().view(torch.int16),
                           torch.nan_to_num(y).contiguous().view(torch.int16))
    for fn in paths.values():                    # warm every path and shape
        time_pass(fn, cs)
    t = {k: [] for k in paths}
    for _ in range(repeats):
        for k, fn in paths.items():
            t[k].append(time_pass(fn, cs))
    C = L * (2 * r + 1)
    res = {"case": name, "B": B, "layout": layout, "channels_last": cl, "dtype": str(dtype).split(".")[-1],
           "lookups_per_pass": len(cs), "out_MB_fp32": B * C * H * W1 * 4 / 1e6,
           "us": {k: {"median": statistics.median(v), "min": min(v), "max": max(v), "repeats": v}
                  for k, v in t.items()}}
    print(json.dumps({k: res[k] for k in ("case", "layout", "channels_last", "dtype")} |
                     {k: round(v["median"], 2) for k, v in res["us"].items()}), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--kitti-batch", type=int, default=64)
    ap.add_argument("--cases", default="kitti,sceneflow")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "outdtype_probe.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("outdtype_probe: needs a HIP device")
    dev = torch.device("cuda", 0)
    out = {"device": torch.cuda.get_device_name(0), "repeats": a.repeats,
           "lib_bytes": os.path.getsize(_lib.LIB_PATH), "cases": []}
    with torch.no_grad():
        for name in a.cases.split(","):
            cfg = bench.CONFIGS[name]
            if name == "kitti":
                cfg = (a.kitti_batch,) + cfg[1:]
                fdt, layout = torch.bfloat16, "records"
            else:
                fdt, layout = torch.float32, "rows"
            inputs = bench.make_inputs(cfg, dev, seed=1, dtype=fdt)
            for cl in (True, False):
                for dtype in (torch.bfloat16, torch.float16):
                    out["cases"].append(run_case(name, cfg, inputs, layout, cl, dtype, a.repeats))
                    torch.cuda.empty_cache()
            del inputs
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
