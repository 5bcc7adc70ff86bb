"""The fused ConvGRU glue (raft-stereo_amd/gru.py) against the
PyTorch ops it replaces, alternated in one process.

  kernels  rc_gru_gates + rc_gru_blend (and the single concatenation of the
           fused route) against the torch op sequence of ConvGRU.forward
           between its convolutions (two concatenations of x, the [r*h, x]
           concatenation, three adds, two sigmoids, tanh, r*h, 1-z, two
           multiplies, an add), at the gru08 / gru16 / gru32 sizes of config 2
           (B = 8, 128 channels, 135x240 / 68x120 / 34x60), fp32 and bf16, NCHW
           and NHWC.  Device-event times over --reps calls, the two sides
           alternated --rounds times: median and min..max of the rounds.  The
           kernels' bytes (7 and 5 operands of N*C*H*W elements) over their
           time, against the 6.29 TB/s measured copy rate of the MI355X.
  e2e      RAFTStereo at 540x960, B = 8, 32 iterations with and without
           fuse_gru (one model, the option toggled, alternated), in one of the
           settings of e2e_probe.py: fp32, bf16 (autocast), bf16_cl (autocast +
           channels_last + MIOpen autotuning); host clock around synchronised
           forwards, per-round times, and the final disparities' difference.

  train_kernels  forward + backward of the same glue: torch autograd of the
           op sequence against the differentiable fused route's pieces (the
           two autograd Functions of gru.py around rc_gru_gates / rc_gru_blend
           and their backward kernels, with the two concatenations that route
           keeps), convolutions excluded: the stacked z/r pre-activations and
           q_pre are leaves, and the gradients the convolutions would send
           into [h, x] and [r*h, x] are given tensors.  Same sizes, dtypes,
           layouts and timing as ``kernels``.  Then the assembly glue, forward
           + backward, at the sizes and parts of ``inputs``: torch autograd of
           pool2x / interp / the casts / the two concatenations ([h, x] and
           [r*h, x], rh a leaf, the two buffers' gradients given tensors)
           against the assembled training route's two Functions (two
           ``gru.assemble`` launches, one ``gru.assemble_backward``); rows
           under ``assembly_rows``, written to profiles/gru_inputs_backward.json
           with the limit of ``inputs``.
  train_step  one training step (forward, loss on every prediction,
           backward) of RAFTStereo with and without the fused GRUs
           (fuse_gru + fuse_gru_backward toggled on one model, alternated), at
           B = 2, 320x720, 22 iterations -- a size whose activations fit next
           to other jobs on one device -- in the settings of ``e2e``; host
           clock around synchronised steps.  ``--toggle inputs_backward``:
           fuse_gru + fuse_gru_backward + fuse_gru_inputs on both sides, with
           and without fuse_gru_inputs_backward (key
           ``train_step_inputs_backward_<setting>`` of
           profiles/gru_inputs_backward.json, with the limit of ``inputs``).

  inputs   the work in front of each ConvGRU call: pool2x / interp of the
           neighbouring scales' states and ``torch.cat(out=)`` into the [h, x]
           buffer (what conv_gru_forward runs without ``fuse_inputs``) against
           one ``gru.assemble`` launch into the same buffer, at the three GRUs'
           sizes and parts of config 2 (gru32: h, pool2x of the 68x120 state;
           gru16: h, pool2x of the 135x240 state, interp of the 34x60 one;
           gru08: h, the motion features -- fp32 in the bf16 rows, as under
           autocast --, interp of the 68x120 state), fp32 and bf16, NCHW and
           NHWC, and gru08 once more as a channels_last network has it: an
           NHWC buffer with NCHW motion features, which the kernel takes one
           element per lane.  Timing as ``kernels``.  The kernel's bytes (dst written
           once, every source read once) over its time against the copy rate,
           and the acceptance test of the change: the assembled side's median
           against the torch side's median * (1 + its own (max - min) / median).

    python tools/gru_probe.py kernels [--out profiles/gru_gates.json]
    python tools/gru_probe.py inputs [--out profiles/gru_inputs.json]
    python tools/gru_probe.py e2e --setting bf16 [--rounds 3]
    python tools/gru_probe.py train_kernels
    python tools/gru_probe.py train_step --setting bf16_cl [--rounds 3]
    python tools/gru_probe.py train_kernels --only assembly
    python tools/gru_probe.py train_step --setting bf16_cl --toggle inputs_backward

Each part merges its results into the --out file under its own key.
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
from raft_stereo_amd import gru  # noqa: E402
from raft_stereo_amd.network import RAFTStereo, StereoArgs  # noqa: E402

COPY_RATE = 6.29e12      # bytes/s, measured copy rate (MI355X_MICROARCH.md)
SIZES = {"gru08": (135, 240, (128, 128)), "gru16": (68, 120, (128, 128)), "gru32": (34, 60, (128,))}


def device_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def alternate(fns, reps, rounds):
    """{name: [ms per call, one per round]} with the callables taking turns."""
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            out[k].append(device_ms(fn, reps))
    return out


def summary(ms):
    return {"median_us": statistics.median(ms) * 1e3, "min_us": min(ms) * 1e3, "max_us": max(ms) * 1e3}


def kernels_part(reps, rounds):
    rows = []
    N, C = 8, 128
    for name, (H, W, parts) in SIZES.items():
        for dt in (torch.float32, torch.bfloat16):
            for cl in (False, True):
                g = torch.Generator(device="cuda").manual_seed(0)
                fmt = torch.channels_last if cl else torch.contiguous_format

                def rnd(ch):
                    t = torch.randn(N, ch, H, W, device="cuda", generator=g).to(dt)
                    return t.contiguous(memory_format=fmt)

                h, zr, ctx, qp = torch.tanh(rnd(C)), rnd(2 * C), rnd(3 * C), rnd(C)
                cz, cr, cq = ctx.split(C, dim=1)
                xs = [rnd(c) for c in parts]
                hx = torch.empty((N, C + sum(parts), H, W), dtype=dt, device="cuda", memory_format=fmt)
                zbuf = torch.empty_like(h)
                hout = torch.empty_like(h)

                def torch_glue():
                    x = torch.cat(xs, dim=1)
                    torch.cat([h, x], dim=1)
                    z = torch.sigmoid(zr[:, :C] + cz)
                    r = torch.sigmoid(zr[:, C:] + cr)
                    torch.cat([r * h, x], dim=1)
                    q = torch.tanh(qp + cq)
                    return (1 - z) * h + z * q

                def fused_glue():
                    torch.cat([h, *xs], dim=1, out=hx)
                    gru.gru_gates(zr[:, :C], zr[:, C:], cz, cr, h, z_out=zbuf, rh_out=hx[:, :C])
                    return gru.gru_blend(zbuf, qp, cq, h, h_out=hout)

                fns = {"torch_glue": torch_glue, "fused_glue": fused_glue,
                       "gates": lambda: gru.gru_gates(zr[:, :C], zr[:, C:], cz, cr, h, z_out=zbuf,
                                                      rh_out=hx[:, :C]),
                       "blend": lambda: gru.gru_blend(zbuf, qp, cq, h, h_out=hout)}
                with torch.no_grad():
                    ms = alternate(fns, reps, rounds)
                row = {"size": name, "shape": [N, C, H, W], "x_channels": list(parts),
                       "dtype": str(dt).replace("torch.", ""), "layout": "NHWC" if cl else "NCHW"}
                for k, v in ms.items():
                    row[k] = summary(v)
                elems = N * C * H * W * h.element_size()
                for k, nops in (("gates", 7), ("blend", 5)):
                    rate = nops * elems / (row[k]["median_us"] * 1e-6)
                    row[k]["bytes"] = nops * elems
                    row[k]["TB_per_s"] = rate / 1e12
                    row[k]["of_copy_rate"] = rate / COPY_RATE
                row["speedup"] = row["torch_glue"]["median_us"] / row["fused_glue"]["median_us"]
                print(json.dumps(row), flush=True)
                rows.append(row)
    return {"reps": reps, "rounds": rounds, "copy_rate_TB_per_s": COPY_RATE / 1e12, "rows": rows}


# (H, W) of h and the x parts of each GRU at config 2: plain (H x W), pooled
# from and resized from a neighbouring scale's state
INPUT_PARTS = {"gru08": ((135, 240), (("plain", (135, 240)), ("resize", (68, 120)))),
               "gru16": ((68, 120), (("pool", (135, 240)), ("resize", (34, 60)))),
               "gru32": ((34, 60), (("pool", (68, 120)),))}


def inputs_part(reps, rounds):
    from raft_stereo_amd import network
    rows = []
    N, C = 8, 128
    for name, ((H, W), parts) in INPUT_PARTS.items():
        for dt in (torch.float32, torch.bfloat16):
            # the third layout is a channels_last network's gru08: its motion
            # features are NCHW (they are concatenated with the NCHW flow)
            for cl, crossed in ((False, False), (True, False)) + (((True, True),) if name == "gru08" else ()):
                g = torch.Generator(device="cuda").manual_seed(0)
                fmt = torch.channels_last if cl else torch.contiguous_format

                def rnd(h, w, dtype, fmt=fmt):
                    t = torch.randn(N, C, h, w, device="cuda", generator=g).to(dtype)
                    return t.contiguous(memory_format=fmt)

                h = torch.tanh(rnd(H, W, dt))
                # the motion features carry the fp32 flow: fp32 under autocast
                srcs = [rnd(sh, sw, torch.float32, torch.contiguous_format if crossed else fmt) if kind == "plain"
                        else rnd(sh, sw, dt) for kind, (sh, sw) in parts]
                hx = torch.empty((N, C * (1 + len(parts)), H, W), dtype=dt, device="cuda", memory_format=fmt)
                hx2 = torch.empty_like(hx)
                lazy = [t if kind == "plain" else gru.Pooled(t) if kind == "pool" else gru.Resized(t, (H, W))
                        for (kind, _), t in zip(parts, srcs)]

                def torch_inputs():
                    xs = [t if kind == "plain" else network.pool2x(t) if kind == "pool" else network.interp(t, h)
                          for (kind, _), t in zip(parts, srcs)]
                    return torch.cat([h, *xs], dim=1, out=hx)

                def assembled():
                    return gru.assemble([h, *lazy], dt, fmt, out=hx2)

                with torch.no_grad():
                    ms = alternate({"torch_inputs": torch_inputs, "assemble": assembled}, reps, rounds)
                    err = (hx2.float() - hx.float()).abs().max().item() / hx.float().abs().max().item()
                row = {"size": name, "shape": [N, C, H, W], "parts": [[k, list(s)] for k, s in parts],
                       "dtype": str(dt).replace("torch.", ""), "layout": ("NHWC, NCHW motion" if crossed else "NHWC") if cl else "NCHW",
                       "norm_err_vs_torch": err}
                for k, v in ms.items():
                    row[k] = summary(v)
                nbytes = hx.numel() * hx.element_size() + sum(t.numel() * t.element_size() for t in [h] + srcs)
                rate = nbytes / (row["assemble"]["median_us"] * 1e-6)
                row["assemble"].update(bytes=nbytes, TB_per_s=rate / 1e12, of_copy_rate=rate / COPY_RATE)
                base = row["torch_inputs"]
                row["speedup"] = base["median_us"] / row["assemble"]["median_us"]
                row["limit_us"] = base["median_us"] * (1 + (base["max_us"] - base["min_us"]) / base["median_us"])
                row["within_limit"] = row["assemble"]["median_us"] <= row["limit_us"]
                print(json.dumps(row), flush=True)
                rows.append(row)
    return {"reps": reps, "rounds": rounds, "copy_rate_TB_per_s": COPY_RATE / 1e12, "rows": rows}


def train_kernels_part(reps, rounds):
    rows = []
    N, C = 8, 128
    for name, (H, W, parts) in SIZES.items():
        for dt in (torch.float32, torch.bfloat16):
            for cl in (False, True):
                g = torch.Generator(device="cuda").manual_seed(0)
                fmt = torch.channels_last if cl else torch.contiguous_format

                def rnd(ch, grad=True):
                    t = torch.randn(N, ch, H, W, device="cuda", generator=g).to(dt)
                    return t.contiguous(memory_format=fmt).requires_grad_(grad)

                h, zr, qp = torch.tanh(rnd(C, False)).requires_grad_(True), rnd(2 * C), rnd(C)
                cz, cr, cq = rnd(C), rnd(C), rnd(C)
                xs = [rnd(c) for c in parts]
                # the unfused route has two convolutions: their outputs are two leaves
                zp, rp = (t.detach().clone(memory_format=fmt).requires_grad_(True) for t in zr.split(C, dim=1))
                leaves = [h, zr, zp, rp, qp, cz, cr, cq, *xs]
                K = C + sum(parts)
                g_out, g_hx, g_rx = rnd(C, False), rnd(K, False), rnd(K, False)

                def step(forward):
                    for t in leaves:
                        t.grad = None
                    out, hx, rx = forward()
                    torch.autograd.backward([out, hx, rx], [g_out, g_hx, g_rx])

                def torch_glue():
                    x = torch.cat(xs, dim=1)
                    hx = torch.cat([h, x], dim=1)
                    z = torch.sigmoid(zp + cz)
                    r = torch.sigmoid(rp + cr)
                    rx = torch.cat([r * h, x], dim=1)
                    q = torch.tanh(qp + cq)
                    return (1 - z) * h + z * q, hx, rx

                def fused_glue():
                    hx = torch.cat([h, *xs], dim=1)
                    z, rh = gru._GatesFn.apply(zr, cz, cr, h)
                    rx = torch.cat([rh, *xs], dim=1)
                    return gru._BlendFn.apply(z, qp, cq, h), hx, rx

                z0, gq = torch.sigmoid(zr[:, :C] + cz).detach(), torch.empty_like(g_out)
                gz, gh, gzr = torch.empty_like(g_out), torch.empty_like(g_out), torch.empty_like(zr.detach())
                fns = {"torch_glue": lambda: step(torch_glue), "fused_glue": lambda: step(fused_glue),
                       "gates_backward": lambda: gru.gru_gates_backward(g_out, g_rx[:, :C], z0, zr.detach()[:, C:],
                                                                        cr.detach(), h.detach(), gzr[:, :C],
                                                                        gzr[:, C:], gh),
                       "blend_backward": lambda: gru.gru_blend_backward(g_out, z0, qp.detach(), cq.detach(),
                                                                        h.detach(), gz, gq, gh)}
                ms = alternate(fns, reps, rounds)
                row = {"size": name, "shape": [N, C, H, W], "x_channels": list(parts),
                       "dtype": str(dt).replace("torch.", ""), "layout": "NHWC" if cl else "NCHW"}
                for k, v in ms.items():
                    row[k] = summary(v)
                elems = N * C * H * W * h.element_size()
                for k, nops in (("gates_backward", 9), ("blend_backward", 8)):
                    rate = nops * elems / (row[k]["median_us"] * 1e-6)
                    row[k]["bytes"] = nops * elems
                    row[k]["TB_per_s"] = rate / 1e12
                    row[k]["of_copy_rate"] = rate / COPY_RATE
                row["speedup"] = row["torch_glue"]["median_us"] / row["fused_glue"]["median_us"]
                print(json.dumps(row), flush=True)
                rows.append(row)
    return {"reps": reps, "rounds": rounds, "copy_rate_TB_per_s": COPY_RATE / 1e12, "rows": rows}


def train_assembly_part(reps, rounds):
    """The assembly glue of the training route, forward + backward."""
    from raft_stereo_amd import network
    rows = []
    N, C = 8, 128
    for name, ((H, W), parts) in INPUT_PARTS.items():
        for dt in (torch.float32, torch.bfloat16):
            for cl in (False, True):
                g = torch.Generator(device="cuda").manual_seed(0)
                fmt = torch.channels_last if cl else torch.contiguous_format

                def rnd(ch, h, w, dtype, grad=True):
                    t = torch.randn(N, ch, h, w, device="cuda", generator=g).to(dtype)
                    return t.contiguous(memory_format=fmt).requires_grad_(grad)

                h, rh = torch.tanh(rnd(C, H, W, dt, False)).requires_grad_(True), rnd(C, H, W, dt)
                # the motion features carry the fp32 flow: fp32 under autocast
                srcs = [rnd(C, sh, sw, torch.float32 if kind == "plain" else dt) for kind, (sh, sw) in parts]
                leaves = [h, rh, *srcs]
                K = C * (1 + len(parts))
                g_hx, g_rx = rnd(K, H, W, dt, False), rnd(K, H, W, dt, False)
                lazy = lambda: [t if kind == "plain" else gru.Pooled(t) if kind == "pool"    # noqa: E731
                                else gru.Resized(t, (H, W)) for (kind, _), t in zip(parts, srcs)]

                def step(forward):
                    for t in leaves:
                        t.grad = None
                    torch.autograd.backward(list(forward()), [g_hx, g_rx])

                def torch_glue():
                    xs = [(t if kind == "plain" else network.pool2x(t) if kind == "pool"
                           else network.interp(t, h)).to(dt) for (kind, _), t in zip(parts, srcs)]
                    hx = torch.cat([h, *xs], dim=1).contiguous(memory_format=fmt)
                    return hx, torch.cat([rh, *xs], dim=1).contiguous(memory_format=fmt)

                def assembled():
                    call = gru._Call()
                    x = lazy()
                    hx = gru._AssembleFn.apply(call, gru._kinds((h, *x)), dt, fmt, h, *srcs)
                    return hx, gru._TailFn.apply(call, fmt, hx, rh)

                meta = gru._parts_meta((h, *lazy()))
                fns = {"torch_glue": lambda: step(torch_glue), "assembled": lambda: step(assembled),
                       "assemble_backward": lambda: gru.assemble_backward(g_hx, meta, (0,), g2=g_rx, g2_from=C)}
                ms = alternate(fns, reps, rounds)
                step(torch_glue)
                want = [t.grad.float().clone() for t in leaves]
                step(assembled)
                err = max(((t.grad.float() - w).abs().max() / w.abs().max()).item() for t, w in zip(leaves, want))
                row = {"size": name, "shape": [N, C, H, W], "parts": [[k, list(s)] for k, s in parts],
                       "dtype": str(dt).replace("torch.", ""), "layout": "NHWC" if cl else "NCHW",
                       "grad_norm_err_vs_torch": err}
                for k, v in ms.items():
                    row[k] = summary(v)
                # both gradients read once, every source's gradient written once
                nbytes = 2 * g_hx.numel() * g_hx.element_size() + sum(t.numel() * t.element_size() for t in srcs)
                rate = nbytes / (row["assemble_backward"]["median_us"] * 1e-6)
                row["assemble_backward"].update(bytes=nbytes, TB_per_s=rate / 1e12, of_copy_rate=rate / COPY_RATE)
                base = row["torch_glue"]
                row["speedup"] = base["median_us"] / row["assembled"]["median_us"]
                row["limit_us"] = base["median_us"] * (1 + (base["max_us"] - base["min_us"]) / base["median_us"])
                row["within_limit"] = row["assembled"]["median_us"] <= row["limit_us"]
                print(json.dumps(row), flush=True)
                rows.append(row)
    return {"reps": reps, "rounds": rounds, "copy_rate_TB_per_s": COPY_RATE / 1e12, "assembly_rows": rows}


def train_step_part(setting, rounds, B=2, H=320, W=720, iters=22, toggle="fuse_gru"):
    mixed, bench, cl = {"fp32": (False, False, False), "bf16": (True, False, False),
                        "bf16_cl": (True, True, True)}[setting]
    torch.backends.cudnn.benchmark = bench
    torch.manual_seed(0)
    args = StereoArgs(mixed_precision=mixed)
    args.autocast_dtype = torch.bfloat16
    inputs = toggle == "inputs_backward"       # both sides fused and assembled; the new option toggled
    model = RAFTStereo(args, fuse_gru=True, fuse_gru_backward=True, fuse_gru_inputs=inputs,
                       fuse_gru_inputs_backward=inputs).eval().cuda()
    if cl:
        model = model.to(memory_format=torch.channels_last)
    grus = [getattr(model.update_block, n) for n in ("gru08", "gru16", "gru32")]
    g = torch.Generator().manual_seed(1234)
    img1 = (torch.rand(B, 3, H, W, generator=g) * 255).cuda()
    img2 = torch.roll(img1, -8, dims=-1)

    def step(fuse):
        for m in grus:
            if inputs:
                m.fuse_inputs_backward = fuse
            else:
                m.fuse = m.fuse_backward = fuse
        model.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        preds = model(img1, img2, iters=iters)
        loss = sum(p[:, 0].float().abs().mean() for p in preds)
        loss.backward()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        grad = torch.cat([p.grad.float().flatten() for p in model.parameters() if p.grad is not None])
        return ms, loss.item(), grad

    ms = {False: [], True: []}
    last = {fuse: step(fuse) for fuse in (False, True)}       # warm-up: every shape of both routes
    torch.cuda.reset_peak_memory_stats()
    peak = {}
    for _ in range(rounds):
        for fuse in (False, True):
            last[fuse] = step(fuse)
            ms[fuse].append(last[fuse][0])
            peak[fuse] = torch.cuda.max_memory_allocated()
            torch.cuda.reset_peak_memory_stats()
    gu, gf = last[False][2], last[True][2]
    res = {"setting": setting, "mixed_bf16": mixed, "miopen_benchmark": bench, "channels_last": cl,
           "shape": [B, H, W], "iters": iters, "rounds": rounds,
           "unfused_ms": ms[False], "fused_ms": ms[True],
           "unfused_median_ms": statistics.median(ms[False]), "fused_median_ms": statistics.median(ms[True]),
           "unfused_peak_GiB": peak[False] / 2 ** 30, "fused_peak_GiB": peak[True] / 2 ** 30,
           "loss_unfused": last[False][1], "loss_fused": last[True][1],
           "grad_norm_err": ((gf - gu).abs().max() / gu.abs().max()).item()}
    res["fused_over_unfused"] = res["fused_median_ms"] / res["unfused_median_ms"]
    if inputs:      # "unfused" is the parent side: the three options without the new one
        res["toggle"] = "fuse_gru_inputs_backward"
        res["limit_ms"] = res["unfused_median_ms"] * (1 + (max(ms[False]) - min(ms[False]))
                                                      / res["unfused_median_ms"])
        res["within_limit"] = res["fused_median_ms"] <= res["limit_ms"]
    print(json.dumps(res), flush=True)
    return res


def e2e_part(setting, rounds, B=8, H=540, W=960, iters=32):
    mixed, bench, cl = {"fp32": (False, False, False), "bf16": (True, False, False),
                        "bf16_cl": (True, True, True)}[setting]
    torch.backends.cudnn.benchmark = bench
    torch.manual_seed(0)
    args = StereoArgs(mixed_precision=mixed)
    args.autocast_dtype = torch.bfloat16
    model = RAFTStereo(args, fuse_gru=True).eval().cuda()
    if cl:
        model = model.to(memory_format=torch.channels_last)
    grus = [getattr(model.update_block, n) for n in ("gru08", "gru16", "gru32")]
    g = torch.Generator().manual_seed(1234)
    img1 = (torch.rand(B, 3, H, W, generator=g) * 255).cuda()
    img2 = torch.roll(img1, -8, dims=-1)

    def forward(fuse):
        for m in grus:
            m.fuse = fuse
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = model(img1, img2, iters=iters)[-1]
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    ms = {False: [], True: []}
    with torch.no_grad():
        last = {fuse: forward(fuse)[1] for fuse in (False, True)}       # warm-up: every shape of both routes
        for _ in range(rounds):
            for fuse in (False, True):
                t, last[fuse] = forward(fuse)
                ms[fuse].append(t)
    diff = (last[True].float() - last[False].float())[:, 0].abs()
    res = {"setting": setting, "mixed_bf16": mixed, "miopen_benchmark": bench, "channels_last": cl,
           "shape": [B, H, W], "iters": iters, "rounds": rounds,
           "unfused_ms": ms[False], "fused_ms": ms[True],
           "unfused_median_ms": statistics.median(ms[False]), "fused_median_ms": statistics.median(ms[True]),
           "final_disparity_mae_px": diff.mean().item(), "final_disparity_max_px": diff.max().item()}
    res["fused_over_unfused"] = res["fused_median_ms"] / res["unfused_median_ms"]
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("part", choices=["kernels", "inputs", "e2e", "train_kernels", "train_step"])
    ap.add_argument("--setting", choices=["fp32", "bf16", "bf16_cl"], default="bf16")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=None)
    ap.add_argument("--only", choices=["gates", "assembly"], default=None,
                    help="train_kernels: the gate glue or the assembly glue alone")
    ap.add_argument("--toggle", choices=["fuse_gru", "inputs_backward"], default="fuse_gru",
                    help="train_step: what the two sides differ in")
    ap.add_argument("--out", default=None, help="profiles/gru_gates.json; profiles/gru_inputs.json for `inputs`; "
                    "profiles/gru_inputs_backward.json for the assembly glue and --toggle inputs_backward")
    a = ap.parse_args()
    new = (a.part == "train_kernels" and a.only == "assembly") or \
        (a.part == "train_step" and a.toggle == "inputs_backward")
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "gru_inputs_backward.json" if new else
                             "gru_inputs.json" if a.part == "inputs" else "gru_gates.json")
    if not torch.cuda.is_available():
        sys.exit("gru_probe: needs a HIP device (no CPU timing)")
    if a.part == "kernels":
        key, res = "kernels", kernels_part(a.reps, a.rounds or 7)
    elif a.part == "inputs":
        key, res = "inputs", inputs_part(a.reps, a.rounds or 7)
    elif a.part == "train_kernels" and a.only == "assembly":
        key, res = "train_kernels", train_assembly_part(a.reps, a.rounds or 7)
    elif a.part == "train_kernels":
        key, res = "train_kernels", train_kernels_part(a.reps, a.rounds or 7)
        if a.only is None:       # the assembly rows go to their own file
            save(os.path.join(ROOT, "profiles", "gru_inputs_backward.json"), "train_kernels",
                 train_assembly_part(a.reps, a.rounds or 7))
    elif a.part == "train_step" and a.toggle == "inputs_backward":
        key, res = f"train_step_inputs_backward_{a.setting}", train_step_part(a.setting, a.rounds or 3,
                                                                               toggle=a.toggle)
    elif a.part == "train_step":
        key, res = f"train_step_{a.setting}", train_step_part(a.setting, a.rounds or 3)
    else:
        key, res = f"e2e_{a.setting}", e2e_part(a.setting, a.rounds or 3)
    save(a.out, key, res)


def save(path, key, res):
    doc = {}
    if os.path.exists(path):
        with open(path) as fh:
            doc = json.load(fh)
    doc[key] = res
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
