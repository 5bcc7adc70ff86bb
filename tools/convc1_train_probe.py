"""Training through the motion encoder's input path: the differentiable fused
lookup + convc1 against the unfused ``relu(convc1(blk(coords)))`` (dev probe,
DESIGN.md §3.2b).

    python tools/convc1_train_probe.py [--shape 8 256 135 240] [--lookups 32] [--reps 7]

One step = build the block from fmaps that require grad, ``lookups`` calls at
different coords (each output kept alive, as convc2 would keep it), one
backward to the fmaps, the conv weight and the bias.  Both paths get the same
seeded inputs and output gradients.  After a warm-up of each, the two are
timed alternately in one process between device events and the medians
printed, with the memory one step of each holds after its forward and its
``torch.cuda.max_memory_allocated``, both above the inputs, the largest
relative difference of the gradients, and the number of ReLU outputs whose
sign differs between the two forwards (the conv sums differ in order).
``--eager-grads`` runs both with ``CorrBlock1D(grad_deferred=False)``.  Needs a
HIP device.
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
from raft_stereo_amd import CorrBlock1D  # noqa: E402


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=4, default=[8, 256, 135, 240], metavar=("B", "D", "H", "W"))
    ap.add_argument("--levels", type=int, default=4)
    ap.add_argument("--radius", type=int, default=4)
    ap.add_argument("--cout", type=int, default=64)
    ap.add_argument("--lookups", type=int, default=32)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--eager-grads", action="store_true",
                    help="CorrBlock1D(grad_deferred=False): every lookup's gradient is added to the level "
                         "gradients at once instead of being held for one deferred pass")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("convc1_train_probe: needs a HIP device")
    B, D, H, W = a.shape
    L, r, cout = a.levels, a.radius, a.cout
    cin = L * (2 * r + 1)
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(11)
    f1 = torch.randn(B, D, H, W, generator=g).to(dev).requires_grad_(True)
    f2 = torch.randn(B, D, H, W, generator=g).to(dev).requires_grad_(True)
    wgt = (torch.randn(cout, cin, 1, 1, generator=g) / cin ** 0.5).to(dev).requires_grad_(True)
    bias = (torch.randn(cout, generator=g) * 0.1).to(dev).requires_grad_(True)
    gout = torch.randn(B, cout, H, W, generator=g).to(dev)
    base = torch.arange(W).float().view(1, 1, 1, W) - torch.rand(B, 1, H, W, generator=g) * 32
    coords = [torch.cat([base + 0.37 * i, torch.zeros_like(base)], 1).to(dev) for i in range(a.lookups)]
    leaves = (wgt, bias, f1, f2)

    def forward(fused):
        blk = CorrBlock1D(f1, f2, num_levels=L, radius=r, grad_deferred=False if a.eager_grads else None)
        if fused:
            return [blk.lookup_convc1(c, wgt, bias, differentiable=True) for c in coords]
        return [torch.relu(F.conv2d(blk(c), wgt, bias)) for c in coords]

    def step(fused, after_forward=None):
        for t in leaves:
            t.grad = None
        outs = forward(fused)
        if after_forward is not None:
            after_forward()
        torch.autograd.backward(outs, [gout] * len(outs))

    paths = {"fused": True, "unfused": False}
    grads = {}
    for name, fused in paths.items():
        for _ in range(a.warmup):
            step(fused)
        grads[name] = [t.grad.clone() for t in leaves]
    torch.cuda.synchronize()
    res = {"shape": a.shape, "levels": L, "radius": r, "cout": cout, "lookups": a.lookups, "reps": a.reps,
           "eager_grads": a.eager_grads}
    for what, x, y in zip(("dW", "db", "df1", "df2"), grads["fused"], grads["unfused"]):
        res[f"{what}_max_diff_rel"] = float((x - y).abs().max() / y.abs().max())
    del grads
    # the two convs sum in different orders, so a pre-activation within rounding
    # of zero can land on either side: such ReLU flips bound the differences above
    with torch.no_grad():
        flips = sum(int(((x > 0) != (y > 0)).sum()) for x, y in zip(forward(True), forward(False)))
    res["relu_sign_flips"] = flips
    res["activations"] = B * cout * H * W * a.lookups

    times = {name: [] for name in paths}
    for _ in range(a.reps):
        for name, fused in paths.items():           # alternate the two paths
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            step(fused)
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1))
    for name in paths:
        res[f"{name}_step_ms"] = round(median(times[name]), 3)
        res[f"{name}_step_min_max_ms"] = [round(min(times[name]), 3), round(max(times[name]), 3)]

    for name, fused in paths.items():
        for t in leaves:
            t.grad = None
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        floor = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        held = []
        step(fused, lambda: held.append(torch.cuda.memory_allocated()))
        torch.cuda.synchronize()
        res[f"{name}_after_forward_above_inputs_MB"] = round((held[0] - floor) / 1e6, 1)
        res[f"{name}_peak_above_inputs_MB"] = round((torch.cuda.max_memory_allocated() - floor) / 1e6, 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
