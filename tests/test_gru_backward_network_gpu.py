"""The training route of the fused ConvGRU (gru.conv_gru_forward(...,
differentiable=True), RAFTStereo(fuse_gru=True, fuse_gru_backward=True),
DESIGN.md §3.7): per module against the float64 module, under autocast against
the unfused route, and through the network against the unfused model and a
"torch twin" that has the fused route's association (the stacked z/r
convolution) and none of its kernels."""
import copy
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from golden_util import norm_err
from raft_stereo_amd import gru
from raft_stereo_amd.network import ConvGRU, RAFTStereo, StereoArgs
from test_gru_network_gpu import DEV, MAE_PX, PARTS, TOL, module_case, small_pair

pytestmark = pytest.mark.gpu
PARAMS = ("convz.weight", "convz.bias", "convr.weight", "convr.bias", "convq.weight", "convq.bias")


class Spies:
    """Counts the calls of the two backward wrappers while active."""

    def __enter__(self):
        self.gates, self.blend = [], []
        self.inner = gru.gru_gates_backward, gru.gru_blend_backward

        def gates(*a, **kw):
            self.gates.append(1)
            return self.inner[0](*a, **kw)

        def blend(*a, **kw):
            self.blend.append(1)
            return self.inner[1](*a, **kw)

        gru.gru_gates_backward, gru.gru_blend_backward = gates, blend
        return self

    def __exit__(self, *exc):
        gru.gru_gates_backward, gru.gru_blend_backward = self.inner


def grad_out(dtype=torch.float32):
    return torch.randn(2, 128, 9, 20, generator=torch.Generator().manual_seed(23)).to(dtype)


def names(kind):
    return ["out", "h", "cz", "cr", "cq"] + [f"x{i}" for i in range(len(PARTS[kind]))] + list(PARAMS)


def forward_backward(m, args, g, route):
    """[output, input gradients, parameter gradients] of one forward +
    backward; ``route(m, *leaves)`` computes the output."""
    leaves = [t.detach().clone(memory_format=torch.preserve_format).requires_grad_(True) for t in args]
    m.zero_grad(set_to_none=True)
    out = route(m, *leaves)
    out.backward(g.to(out.device))
    got = [out.detach()] + [t.grad for t in leaves] + [dict(m.named_parameters())[n].grad for n in PARAMS]
    assert all(t is not None for t in got)
    return [t.detach().clone() for t in got]


@functools.lru_cache(maxsize=None)
def reference64(kind):
    """The same module in float64 on the CPU; never modified."""
    m, args = module_case(kind)
    m64 = copy.deepcopy(m).double().cpu()
    return [t.numpy() for t in forward_backward(m64, [t.double().cpu() for t in args], grad_out().double(),
                                                lambda mod, *a: mod(*a))]


def differentiable(mod, *a):
    return gru.conv_gru_forward(mod, *a, differentiable=True)


@pytest.mark.parametrize("channels_last", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("kind", sorted(PARTS))
def test_module_fp32(kind, channels_last, monkeypatch):
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    m, args = module_case(kind, channels_last)
    m.requires_grad_(True)
    ref = reference64(kind)
    keep = [t.clone() for t in args]
    assert gru.why_not_fusable(m, *[t.clone().requires_grad_(True) for t in args], differentiable=True) is None
    with Spies() as spies:
        got = forward_backward(m, args, grad_out(), differentiable)
    assert len(spies.gates) == 1 and len(spies.blend) == 1, (len(spies.gates), len(spies.blend))
    assert all(torch.equal(a, b) for a, b in zip(args, keep)), "an input was modified"
    for g, r, n in zip(got, ref, names(kind)):
        assert tuple(g.shape) == r.shape and g.dtype == torch.float32, n
        err = norm_err(g.cpu().numpy(), r)
        print(f"{kind} fp32 {n}: norm_err vs float64 {err:.2e}")
        assert err <= TOL, (n, err)
    # the same convolutions and the same forward kernels as the inference route
    with torch.no_grad():
        inference = gru.conv_gru_forward(m, *args)
    assert torch.equal(got[0], inference), "the differentiable route's forward differs from the inference route's"
    assert gru._classes(got[0]) & gru._classes(args[0]), "the new state is not in h's layout"
    # the module takes the route only with both attributes set
    m.fuse = True
    with Spies() as spies:
        forward_backward(m, args, grad_out(), lambda mod, *a: mod(*a))
        assert not spies.gates and not spies.blend
        m.fuse_backward = True
        via = forward_backward(m, args, grad_out(), lambda mod, *a: mod(*a))
    assert len(spies.gates) == 1 and len(spies.blend) == 1
    assert torch.equal(via[0], got[0])
    assert all(norm_err(a.cpu().numpy(), r) <= TOL for a, r in zip(via, ref))


def test_differentiable_with_nothing_to_record_is_the_inference_route():
    m, args = module_case("gru16")
    with torch.no_grad():
        want = gru.conv_gru_forward(m, *args)
        with Spies() as spies:
            got = gru.conv_gru_forward(m, *args, differentiable=True)
    m.requires_grad_(False)
    frozen = gru.conv_gru_forward(m, *args, differentiable=True)      # grad mode, nothing requires grad
    assert not spies.gates and not frozen.requires_grad and got.grad_fn is None
    assert torch.equal(got, want) and torch.equal(frozen, want)


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("kind", sorted(PARTS))
def test_module_autocast(kind, dt, monkeypatch):
    """The gradients of both routes under autocast against the fp32 module's
    on the same (dtype-rounded) inputs: the fused route's error is at most
    1.25 times the unfused route's for every gradient, the factor
    test_gru_network_gpu.py::test_module_autocast uses for the outputs."""
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    m, args = module_case(kind)
    m.requires_grad_(True)
    low = [t.to(dt) for t in args]
    if kind == "gru08":
        low[4] = low[4].float()             # the motion features stay fp32 under autocast
    ref = forward_backward(m, [t.float() for t in low], grad_out(), lambda mod, *a: mod(*a))
    with torch.autocast("cuda", dtype=dt):
        assert gru.why_not_fusable(m, *[t.clone().requires_grad_(True) for t in low], differentiable=True) is None
    g = grad_out(dt)

    def under_autocast(route):
        def run(mod, *a):
            with torch.autocast("cuda", dtype=dt):
                return route(mod, *a)
        return run

    unfused = forward_backward(m, low, g, under_autocast(lambda mod, *a: mod(*a)))
    with Spies() as spies:
        fused = forward_backward(m, low, g, under_autocast(differentiable))
    assert len(spies.gates) == 1 and len(spies.blend) == 1
    bad = []
    for f, u, r, n in zip(fused, unfused, ref, names(kind)):
        assert f.dtype == u.dtype and f.shape == u.shape == r.shape, n
        e_f = norm_err(f.float().cpu().numpy(), r.cpu().numpy())
        e_u = norm_err(u.float().cpu().numpy(), r.cpu().numpy())
        print(f"{kind} {dt} {n}: norm_err vs fp32 fused {e_f:.3e}, unfused {e_u:.3e}, ratio {e_f / e_u:.2f}")
        # the output is printed only: test_gru_network_gpu.py::test_module_autocast bounds it
        if n != "out" and not e_f <= 1.25 * e_u:
            bad.append((n, e_f, e_u))
    assert not bad, bad


def twin_forward(self, h, cz, cr, cq, *x_list):
    """ConvGRU.forward with convz and convr stacked, as the fused route runs
    them, and torch elementwise ops."""
    w, b, C = gru._zr_conv(self)
    zr = F.conv2d(torch.cat([h, *x_list], dim=1), w, b, padding=self.convz.padding, dilation=self.convz.dilation)
    z = torch.sigmoid(zr[:, :C] + cz)
    r = torch.sigmoid(zr[:, C:] + cr)
    q = torch.tanh(self.convq(torch.cat([r * h, *x_list], dim=1)) + cq)
    return (1 - z) * h + z * q


@functools.lru_cache(maxsize=None)
def training_run(which):
    """(predictions, parameter gradients, calls of the two backward wrappers)
    of one training step at 64x96, 2 iterations, fp32, deterministic
    convolutions."""
    kw = {"unfused": {}, "twin": {}, "fused": dict(fuse_gru=True, fuse_gru_backward=True),
          "forward only": dict(fuse_gru=True)}[which]
    det, orig = torch.backends.cudnn.deterministic, ConvGRU.forward
    torch.backends.cudnn.deterministic = True
    if which == "twin":
        ConvGRU.forward = twin_forward
    try:
        torch.manual_seed(0)
        model = RAFTStereo(StereoArgs(), **kw).eval().to(DEV)
        with Spies() as spies:
            preds = model(*small_pair(), iters=2)
            preds[-1][:, 0].abs().mean().backward()
    finally:
        torch.backends.cudnn.deterministic, ConvGRU.forward = det, orig
    grads = {n: p.grad.cpu() for n, p in model.named_parameters() if p.grad is not None}
    return [p.detach().cpu() for p in preds], grads, (len(spies.gates), len(spies.blend))


def test_network_runs_both_backward_kernels_per_gru_call():
    assert training_run("fused")[2] == (6, 6)              # 3 GRUs x 2 iterations
    assert training_run("forward only")[2] == (0, 0)
    assert training_run("unfused")[2] == (0, 0)


def test_network_predictions_and_gradients():
    pu, gu, _ = training_run("unfused")
    pf, gf, _ = training_run("fused")
    _, gt, _ = training_run("twin")
    assert len(pf) == len(pu)
    for i, (p, q) in enumerate(zip(pf, pu)):
        mae = (p - q).abs().mean().item()
        print(f"iteration {i}: fused vs unfused MAE {mae:.3e} px")
        assert mae <= MAE_PX, (i, mae)
    assert gf.keys() == gu.keys() == gt.keys() and any("gru08.convq" in n for n in gf)
    for n in gu:
        assert gf[n].shape == gu[n].shape and gf[n].dtype == gu[n].dtype, n
        assert torch.isfinite(gf[n]).all(), n
    # parameters whose gradient is mathematically zero (a conv bias in front
    # of an InstanceNorm): rounding noise only, nothing to compare
    top = max(g.abs().max().item() for g in gu.values())
    zero = [n for n in gu if gu[n].abs().max().item() < 1e-8 * top]
    print(f"{len(gu)} parameters, largest max|g| {top:.3e}; left out as zero: {zero}")
    assert len(zero) <= 4, zero
    worst = ("", 0.0)
    for n in gu:
        if n in zero:
            continue
        e_t = norm_err(gf[n].numpy(), gt[n].numpy())
        e_u = norm_err(gf[n].numpy(), gu[n].numpy())
        worst = max(worst, (n, e_u), key=lambda t: t[1])
        assert e_t <= TOL, (n, e_t)
    print(f"worst per-parameter norm_err fused vs unfused: {worst[1]:.2e} ({worst[0]})")

    def flat(g):
        return np.concatenate([g[n].numpy().ravel() for n in gu])

    e_all = norm_err(flat(gf), flat(gu))
    print(f"all parameters concatenated: fused vs unfused {e_all:.2e}, twin vs unfused "
          f"{norm_err(flat(gt), flat(gu)):.2e}")
    assert e_all <= TOL, e_all
