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

``--compare-test-mode SETTING`` times the three ways to a disparity on one
model (built with ``fuse_gru`` and ``fuse_gru_inputs``): ``forward()``,
``forward(upsample=True)`` and ``forward(test_mode=True)``, alternated the same
way; ``limit_ms`` is the ``forward()`` route's median plus its own spread.  It
also records the difference between the test-mode ``flow_up`` and the last
prediction of ``upsample=True``.  Merged into ``--out`` (default
``profiles/test_mode.json``) under ``e2e_SETTING``.

    python tools/e2e_probe.py --compare-test-mode bf16_cl [--rounds 3]
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


def compare_test_mode(setting, rounds, B=8, H=540, W=960, iters=32):
    """forward(), forward(upsample=True) and forward(test_mode=True) on one model."""
    mixed, bench, cl = SETTINGS[setting]
    model, img1, img2 = build(mixed, bench, cl, B, H, W, fuse_gru=True, fuse_gru_inputs=True)
    routes = {"forward": {}, "upsample": {"upsample": True}, "test_mode": {"test_mode": True}}

    def forward(route):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = model(img1, img2, iters=iters, **routes[route])[-1]
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    ms = {r: [] for r in routes}
    with torch.no_grad():
        last = {r: forward(r)[1] for r in routes}                        # warm-up: every shape of every route
        for _ in range(rounds):
            for r in routes:
                t, last[r] = forward(r)
                ms[r].append(t)
    diff = (last["test_mode"].float() - last["upsample"].float()).abs()
    base = ms["forward"]
    med = statistics.median(base)
    res = {"setting": setting, "mixed_bf16": mixed, "miopen_benchmark": bench, "channels_last": cl,
           "fuse_gru": True, "fuse_gru_inputs": True, "shape": [B, H, W], "iters": iters, "rounds": rounds,
           **{f"{r}_ms": ms[r] for r in routes}, **{f"{r}_median_ms": statistics.median(ms[r]) for r in routes},
           "limit_ms": med * (1 + (max(base) - min(base)) / med),
           "flow_up_mae_px": diff.mean().item(), "flow_up_max_px": diff.max().item()}
    res["test_mode_over_forward"] = res["test_mode_median_ms"] / med
    res["test_mode_over_upsample"] = res["test_mode_median_ms"] / res["upsample_median_ms"]
    res["within_limit"] = res["test_mode_median_ms"] <= res["limit_ms"]
    return res


def merge(path, key, res):
    doc = {}
    if os.path.exists(path):
        with open(path) as fh:
            doc = json.load(fh)
    doc[key] = res
    with open(path, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--fuse-gru", action="store_true", help="RAFTStereo(fuse_gru=True)")
    ap.add_argument("--fuse-gru-inputs", action="store_true", help="RAFTStereo(fuse_gru_inputs=True); needs --fuse-gru")
    ap.add_argument("--compare-inputs", choices=sorted(SETTINGS), default=None, metavar="SETTING")
    ap.add_argument("--any-format", action="store_true", help="with --compare-inputs: fuse_inputs = 'any'")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--compare-test-mode", choices=sorted(SETTINGS), default=None, metavar="SETTING")
    ap.add_argument("--out", default=None, help="default: profiles/gru_inputs.json, or profiles/test_mode.json "
                    "with --compare-test-mode")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("e2e_probe: needs a HIP device (no CPU timing)")
    if a.compare_test_mode:
        res = compare_test_mode(a.compare_test_mode, a.rounds)
        print(json.dumps(res), flush=True)
        merge(a.out or os.path.join(ROOT, "profiles", "test_mode.json"), f"e2e_{a.compare_test_mode}", res)
        return
    if a.compare_inputs:
        res = compare_inputs(a.compare_inputs, a.rounds, any_format=a.any_format)
        print(json.dumps(res), flush=True)
        merge(a.out or os.path.join(ROOT, "profiles", "gru_inputs.json"),
              f"e2e_{a.compare_inputs}" + ("_any" if a.any_format else ""), res)
        return
    flags = {k: True for k, on in (("fuse_gru", a.fuse_gru), ("fuse_gru_inputs", a.fuse_gru_inputs)) if on}
    for mixed, bench, cl in [(False, False, False), (False, True, False), (True, False, False),
                             (True, True, False), (True, True, True)]:
        print(json.dumps(run(mixed, bench, cl, a.steps, **flags)), flush=True)


if __name__ == "__main__":
    main()
