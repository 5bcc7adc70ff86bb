"""Whole-network timing at config 2 under different PyTorch execution settings
(encoders/GRU stay PyTorch ops; only how they run changes).

    python tools/e2e_probe.py [--steps 2] [--fuse-gru] [--fuse-gru-inputs]

``--fuse-gru`` / ``--fuse-gru-inputs`` build the network with those options
(DESIGN.md §3.7).  ``--compare-inputs SETTING`` times what ``fuse_gru_inputs``
adds to ``fuse_gru``: one model built with both, the ``fuse_inputs``
attributes toggled, the two sides alternated for ``--rounds`` rounds of one
synchronised forward each after a warm-up of both, in one of the settings fp32,
bf16 (autocast) and bf16_cl (autocast + channels_last + MIOpen autotuning);
the result is merged into ``--out`` under ``e2e_SETTING``.  ``--any-format``
sets ``fuse_inputs = "any"`` on that side: every GRU is assembled, also where
a part is in another memory format than the buffer (gru08 of a channels_last
network), which ``fuse_gru_inputs=True`` leaves to the PyTorch ops; the key is
``e2e_SETTING_any``.

    python tools/e2e_probe.py --compare-inputs bf16_cl [--rounds 3] [--out profiles/gru_inputs.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pkgload  # noqa: E402

pkgload.load()
from raft_stereo_amd.network import RAFTStereo, StereoArgs  # noqa: E402


SETTINGS = {"fp32": (False, False, False), "bf16": (True, False, False), "bf16_cl": (True, True, True)}


def build(mixed, benchmark, channels_last, B, H, W, **flags):
    torch.backends.cudnn.benchmark = benchmark
    torch.manual_seed(0)
    args = StereoArgs(mixed_precision=mixed)
    args.autocast_dtype = torch.bfloat16
    model = RAFTStereo(args, **flags).eval().cuda()
    if channels_last:
        model = model.to(memory_format=torch.channels_last)
    g = torch.Generator().manual_seed(1234)
    img1 = (torch.rand(B, 3, H, W, generator=g) * 255).cuda()
    img2 = torch.roll(img1, -8, dims=-1)
    return model, img1, img2


def run(mixed, benchmark, channels_last, steps, B=8, H=540, W=960, iters=32, **flags):
    model, img1, img2 = build(mixed, benchmark, channels_last, B, H, W, **flags)
    with torch.no_grad():
        model(img1, img2, iters=iters)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            model(img1, img2, iters=iters)
        torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    return {"mixed_bf16": mixed, "miopen_benchmark": benchmark, "channels_last": channels_last, **flags,
            "ms_per_batch": dt * 1e3, "pairs_per_s": B / dt}


def compare_inputs(setting, rounds, B=8, H=540, W=960, iters=32, any_format=False):
    """fuse_gru alone against fuse_gru + fuse_gru_inputs on one model."""
    mixed, bench, cl = SETTINGS[setting]
    model, img1, img2 = build(mixed, bench, cl, B, H, W, fuse_gru=True, fuse_gru_inputs=True)
    ub = model.update_block
    mods = [ub, ub.gru08, ub.gru16, ub.gru32]

    def forward(inputs):
        for m in mods:
            m.fuse_inputs = "any" if inputs and any_format else inputs
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = model(img1, img2, iters=iters)[-1]
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    ms = {False: [], True: []}
    with torch.no_grad():
        last = {side: forward(side)[1] for side in (False, True)}       # warm-up: every shape of both routes
        for _ in range(rounds):
            for side in (False, True):
                t, last[side] = forward(side)
                ms[side].append(t)
    diff = (last[True].float() - last[False].float())[:, 0].abs()
    base = ms[False]
    med = statistics.median(base)
    res = {"setting": setting, "mixed_bf16": mixed, "miopen_benchmark": bench, "channels_last": cl,
           "any_format": any_format, "shape": [B, H, W], "iters": iters, "rounds": rounds,
           "fuse_gru_ms": base, "fuse_gru_inputs_ms": ms[True],
           "fuse_gru_median_ms": med, "fuse_gru_inputs_median_ms": statistics.median(ms[True]),
           "limit_ms": med * (1 + (max(base) - min(base)) / med),
           "final_disparity_mae_px": diff.mean().item(), "final_disparity_max_px": diff.max().item()}
    res["inputs_over_fuse_gru"] = res["fuse_gru_inputs_median_ms"] / med
    res["within_limit"] = res["fuse_gru_inputs_median_ms"] <= res["limit_ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--fuse-gru", action="store_true", help="RAFTStereo(fuse_gru=True)")
    ap.add_argument("--fuse-gru-inputs", action="store_true", help="RAFTStereo(fuse_gru_inputs=True); needs --fuse-gru")
    ap.add_argument("--compare-inputs", choices=sorted(SETTINGS), default=None, metavar="SETTING")
    ap.add_argument("--any-format", action="store_true", help="with --compare-inputs: fuse_inputs = 'any'")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gru_inputs.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("e2e_probe: needs a HIP device (no CPU timing)")
    if a.compare_inputs:
        res = compare_inputs(a.compare_inputs, a.rounds, any_format=a.any_format)
        print(json.dumps(res), flush=True)
        doc = {}
        if os.path.exists(a.out):
            with open(a.out) as fh:
                doc = json.load(fh)
        doc[f"e2e_{a.compare_inputs}" + ("_any" if a.any_format else "")] = res
        with open(a.out, "w") as fh:
            json.dump(doc, fh, indent=1)
            fh.write("\n")
        return
    flags = {k: True for k, on in (("fuse_gru", a.fuse_gru), ("fuse_gru_inputs", a.fuse_gru_inputs)) if on}
    for mixed, bench, cl in [(False, False, False), (False, True, False), (True, False, False),
                             (True, True, False), (True, True, True)]:
        print(json.dumps(run(mixed, bench, cl, a.steps, **flags)), flush=True)


if __name__ == "__main__":
    main()
