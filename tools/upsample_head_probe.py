"""The upsampling head against the route it replaces, kernel level.

    python tools/upsample_head_probe.py [--reps 20] [--rounds 5] [--out profiles/test_mode.json]

At the size of config 2's last step (N = 8, C = 1, 135 x 240, f = 4) and for a
mask as the update block writes it in fp32 NCHW, bf16 NCHW and bf16
channels-last, two callables take turns:

  head      upsample.upsample_head(flow, mask, 4, 0.25): one launch;
  composed  upsample.convex_upsample(flow, 0.25 * mask, 4), what
            forward(upsample=True) runs for one prediction, with the scale pass
            and the wrapper's cast and layout copy.

Device time by events around ``--reps`` calls, ``--rounds`` rounds, medians.
Each row also holds each side's algorithmic bytes (mask + flow + out, the mask
in its own dtype; the same for both sides) over its time, as a fraction of the
6.29 TB/s copy rate, and whether the outputs are bit-equal.  Merged into
``--out`` under ``kernel_CASE``.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pkgload  # noqa: E402

pkgload.load()
from raft_stereo_amd.upsample import convex_upsample, upsample_head  # noqa: E402

COPY_RATE = 6.29e12      # bytes/s, measured copy rate (MI355X_MICROARCH.md)
N, C, H, W, F = 8, 1, 135, 240, 4
CASES = {"fp32": (torch.float32, False), "bf16": (torch.bfloat16, False), "bf16_cl": (torch.bfloat16, True)}


def device_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def probe(case, reps, rounds):
    dtype, cl = CASES[case]
    g = torch.Generator().manual_seed(7)
    flow2 = (torch.randn(N, 2, H, W, generator=g) * 5).cuda()
    mask = (torch.randn(N, 9 * F * F, H, W, generator=g) * 2).to(dtype).cuda()
    if cl:
        mask = mask.contiguous(memory_format=torch.channels_last)
    flow = flow2[:, :1]
    fns = {"head": lambda: upsample_head(flow, mask, F, 0.25),
           "composed": lambda: convex_upsample(flow, 0.25 * mask, F)}
    with torch.no_grad():
        outs = {k: fn() for k, fn in fns.items()}
        torch.cuda.synchronize()
        ms = {k: [] for k in fns}
        for _ in range(rounds):
            for k, fn in fns.items():
                ms[k].append(device_ms(fn, reps))
    nbytes = mask.numel() * mask.element_size() + N * C * H * W * 4 + N * C * F * H * F * W * 4
    row = {"case": case, "shape": [N, C, H, W], "factor": F, "reps": reps, "rounds": rounds,
           "algorithmic_bytes": nbytes, "bit_equal": bool(torch.equal(outs["head"], outs["composed"]))}
    for k in fns:
        med = statistics.median(ms[k])
        row[f"{k}_us"] = [t * 1e3 for t in ms[k]]
        row[f"{k}_median_us"] = med * 1e3
        row[f"{k}_of_copy_rate"] = nbytes / (med * 1e-3) / COPY_RATE
    row["head_over_composed"] = row["head_median_us"] / row["composed_median_us"]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "test_mode.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("upsample_head_probe: needs a HIP device (no CPU timing)")
    doc = {}
    if os.path.exists(a.out):
        with open(a.out) as fh:
            doc = json.load(fh)
    for case in CASES:
        row = probe(case, a.reps, a.rounds)
        print(json.dumps(row), flush=True)
        doc[f"kernel_{case}"] = row
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
