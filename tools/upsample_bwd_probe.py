"""Convex upsampler forward + backward: the HIP autograd function against the
unfold + softmax formulation in torch ops (dev probe).

    python tools/upsample_bwd_probe.py [--shape 8 1 135 240 4] [--reps 30]

Both paths get the same seeded inputs and output gradient.  After a warm-up of
each, the two are timed alternately between device events (one forward +
backward per sample) and the medians printed, then the peak device memory of
one step of each above the inputs, then the HIP backward alone with its
bytes-model time at the measured HBM rate.  Needs a HIP device.
"""
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
from raft_stereo_amd.upsample import convex_upsample  # noqa: E402

HBM_BYTES_PER_S = 6.29e12     # measured streaming rate the project uses


def torch_upsample(flow, mask, f):
    """RAFT-Stereo's formulation: autograd keeps the (N, C, 9, f, f, H, W)
    product, the softmax and the unfolded flow for the backward."""
    N, C, H, W = flow.shape
    m = torch.softmax(mask.view(N, 1, 9, f, f, H, W), dim=2)
    up = F.unfold(f * flow, [3, 3], padding=1).view(N, C, 9, 1, 1, H, W)
    up = torch.sum(m * up, dim=2)
    return up.permute(0, 1, 4, 2, 5, 3).reshape(N, C, f * H, f * W)


def bwd_model_bytes(N, C, H, W, f):
    """HBM bytes of rc_convex_upsample_backward per the kernels' design: mask,
    grad_out and flow read once, grad_mask and grad_flow written once, the
    workspace written and read once."""
    per_pixel = (9 * f * f + f * f * C + C) + (9 * f * f + C) + 2 * 9 * C
    return 4 * per_pixel * N * H * W


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=5, default=[8, 1, 135, 240, 4],
                    metavar=("N", "C", "H", "W", "F"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("upsample_bwd_probe: needs a HIP device")
    N, C, H, W, f = a.shape
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(5)
    flow = (torch.randn(N, C, H, W, generator=g) * 5).to(dev).requires_grad_(True)
    mask = (torch.randn(N, 9 * f * f, H, W, generator=g) * 2).to(dev).requires_grad_(True)
    gout = torch.randn(N, C, f * H, f * W, generator=g).to(dev)

    def step(fn, backward=True):
        flow.grad = mask.grad = None
        out = fn(flow, mask, f)
        if backward:
            out.backward(gout)

    paths = {"hip": lambda fl, mk, ff: convex_upsample(fl, mk, ff, differentiable=True),
             "torch": torch_upsample}
    grads = {}
    for name, fn in paths.items():
        for _ in range(a.warmup):
            step(fn)
        grads[name] = (flow.grad.clone(), mask.grad.clone())
    torch.cuda.synchronize()
    res = {"shape": a.shape, "reps": a.reps}
    # same results before any time is compared
    for i, what in enumerate(("grad_flow", "grad_mask")):
        ref = grads["torch"][i]
        res[f"{what}_max_diff_rel"] = float((grads["hip"][i] - ref).abs().max() / ref.abs().max())

    times = {name: [] for name in paths}
    fwd = {name: [] for name in paths}
    for _ in range(a.reps):
        for name, fn in paths.items():          # alternate the two paths
            for bucket, backward in ((times, True), (fwd, False)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                step(fn, backward)
                e1.record()
                torch.cuda.synchronize()
                bucket[name].append(e0.elapsed_time(e1))
    for name in paths:
        res[f"{name}_fwd_bwd_ms"] = round(median(times[name]), 4)
        res[f"{name}_fwd_ms"] = round(median(fwd[name]), 4)
        res[f"{name}_fwd_bwd_min_max_ms"] = [round(min(times[name]), 4), round(max(times[name]), 4)]

    for name, fn in paths.items():
        flow.grad = mask.grad = None
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        step(fn)
        torch.cuda.synchronize()
        res[f"{name}_peak_above_inputs_MB"] = round((torch.cuda.max_memory_allocated() - base) / 1e6, 1)

    # the HIP backward alone (both kernels), against its bytes model
    out = convex_upsample(flow, mask, f, differentiable=True)
    bwd = []
    for _ in range(a.warmup + a.reps):
        flow.grad = mask.grad = None
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out.backward(gout, retain_graph=True)
        e1.record()
        torch.cuda.synchronize()
        bwd.append(e0.elapsed_time(e1))
    t = median(bwd[a.warmup:])
    model = bwd_model_bytes(N, C, H, W, f)
    res["hip_bwd_ms"] = round(t, 4)
    res["hip_bwd_model_MB"] = round(model / 1e6, 2)
    res["hip_bwd_model_ms_at_6.29TBps"] = round(model / HBM_BYTES_PER_S * 1e3, 4)
    res["hip_bwd_fraction_of_hbm_rate"] = round(model / HBM_BYTES_PER_S / (t * 1e-3), 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
