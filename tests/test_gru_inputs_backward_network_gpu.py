"""The assembled training route of the fused ConvGRU
(``ConvGRU.fuse_inputs_backward``, RAFTStereo(fuse_gru_inputs_backward=True),
DESIGN.md §3.7): [h, x] and [r*h, x] from ``gru.assemble``, their backward one
``gru.assemble_backward`` launch.  Per module against the float64 module, under
autocast against the unfused route, and through the network against the
unfused model."""
import copy
import functools

import numpy as np
import pytest
import torch

from golden_util import norm_err
from raft_stereo_amd import gru
from raft_stereo_amd.network import RAFTStereo, StereoArgs
from test_gru_backward_network_gpu import PARAMS, forward_backward, grad_out
from test_gru_inputs_network_gpu import PARTS, module_case
from test_gru_network_gpu import DEV, MAE_PX, TOL, small_pair

pytestmark = pytest.mark.gpu
ALL = dict(fuse_gru=True, fuse_gru_backward=True, fuse_gru_inputs=True, fuse_gru_inputs_backward=True)


class Spies:
    """Records the calls of gru.assemble and gru.assemble_backward while
    active: ``backward`` holds the spatial size of each call's gradient."""

    def __enter__(self):
        self.assemble, self.backward = [], []
        self.inner = gru.assemble, gru.assemble_backward

        def assemble(*a, **kw):
            self.assemble.append(1)
            return self.inner[0](*a, **kw)

        def backward(g, *a, **kw):
            self.backward.append(tuple(g.shape[2:]))
            return self.inner[1](g, *a, **kw)

        gru.assemble, gru.assemble_backward = assemble, backward
        return self

    def __exit__(self, *exc):
        gru.assemble, gru.assemble_backward = self.inner


def names(kind):
    return ["out", "h", "cz", "cr", "cq"] + [f"src{i}" for i in range(len(PARTS[kind]))] + list(PARAMS)


def case(kind, channels_last=False):
    """(module with every attribute of the route set, inputs, and as functions
    of (module, *inputs): the route called directly, the unfused body on
    materialised parts, the module called with the descriptors)."""
    m, state, srcs, lazy = module_case(kind, channels_last)
    m.requires_grad_(True)
    m.fuse = m.fuse_backward = m.fuse_inputs = m.fuse_inputs_backward = True

    def assembled(mod, *a):
        return gru.conv_gru_forward(mod, *a[:4], *lazy(list(a[4:])), differentiable=True)

    def plain(mod, *a):
        was, mod.fuse = mod.fuse, False
        try:
            return mod(*a[:4], *gru.materialized(lazy(list(a[4:]))))
        finally:
            mod.fuse = was

    def module(mod, *a):
        return mod(*a[:4], *lazy(list(a[4:])))

    return m, state + srcs, assembled, plain, module


@functools.lru_cache(maxsize=None)
def reference64(kind):
    """The same module in float64 on the CPU, pool2x and interp by the PyTorch
    ops; never modified."""
    m, args, _, plain, _ = case(kind)
    m64 = copy.deepcopy(m).double().cpu()
    return [t.numpy() for t in forward_backward(m64, [t.double().cpu() for t in args], grad_out().double(), plain)]


@pytest.mark.parametrize("channels_last", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("kind", sorted(PARTS))
def test_module_fp32(kind, channels_last, monkeypatch):
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    m, args, assembled, _, module = case(kind, channels_last)
    ref = reference64(kind)
    keep = [t.clone() for t in args]
    with Spies() as spies:
        got = forward_backward(m, args, grad_out(), assembled)
    assert len(spies.backward) == 1 and len(spies.assemble) == 2, (spies.backward, len(spies.assemble))
    assert all(torch.equal(a, b) for a, b in zip(args, keep)), "an input was modified"
    for g, r, n in zip(got, ref, names(kind)):
        assert tuple(g.shape) == r.shape and g.dtype == torch.float32, n
        err = norm_err(g.cpu().numpy(), r)
        print(f"{kind} fp32 {n}: norm_err vs float64 {err:.2e}")
        assert err <= TOL, (n, err)
    with torch.no_grad():
        with Spies() as spies:
            inference = assembled(m, *args)
    assert len(spies.assemble) == 1 and not spies.backward
    assert torch.equal(got[0], inference), "the training route's forward differs from the inference route's"
    # the module takes the route by its attributes, and leaves it without the new one
    with Spies() as spies:
        via = forward_backward(m, args, grad_out(), module)
        assert len(spies.backward) == 1
        m.fuse_inputs_backward = False
        forward_backward(m, args, grad_out(), module)
        assert len(spies.backward) == 1 and len(spies.assemble) == 2
    assert torch.equal(via[0], got[0])


@pytest.mark.parametrize("kind", sorted(PARTS))
def test_partial_gradients(kind, monkeypatch):
    """A frozen convq, and h as the only leaf that requires a gradient: the
    float64 gradients all the same."""
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    m, args, assembled, _, _ = case(kind)
    ref = dict(zip(names(kind), reference64(kind)))
    m.convq.requires_grad_(False)
    leaves = [t.detach().clone().requires_grad_(True) for t in args]
    m.zero_grad(set_to_none=True)
    assembled(m, *leaves).backward(grad_out().to(DEV))
    got = dict(zip(names(kind)[1:], [t.grad for t in leaves] + [dict(m.named_parameters())[n].grad for n in PARAMS]))
    assert got["convq.weight"] is None and got["convq.bias"] is None
    for n, g in got.items():
        if g is not None:
            assert norm_err(g.cpu().numpy(), ref[n]) <= TOL, n
    m.requires_grad_(False)
    h = args[0].detach().clone().requires_grad_(True)
    with Spies() as spies:
        assembled(m, h, *args[1:]).backward(grad_out().to(DEV))
    assert not spies.backward, "no source asks for a gradient: h's is a slice"
    assert norm_err(h.grad.cpu().numpy(), ref["h"]) <= TOL
    # and the sources alone
    srcs = [t.detach().clone().requires_grad_(True) for t in args[4:]]
    with Spies() as spies:
        assembled(m, *args[:4], *srcs).backward(grad_out().to(DEV))
    assert len(spies.backward) == 1
    for i, t in enumerate(srcs):
        assert norm_err(t.grad.cpu().numpy(), ref[f"src{i}"]) <= TOL, i


def test_second_backward_with_retain_graph(monkeypatch):
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    m, args, assembled, _, _ = case("gru16")
    leaves = [t.detach().clone().requires_grad_(True) for t in args]
    out = assembled(m, *leaves)
    g = grad_out().to(DEV)
    tensors = leaves + list(m.parameters())
    with Spies() as spies:
        first = torch.autograd.grad(out, tensors, g, retain_graph=True)
        second = torch.autograd.grad(out, tensors, g)
    assert len(spies.backward) == 2
    ref = reference64("gru16")
    for a, b, r, n in zip(first, second, ref[1:], names("gru16")[1:]):
        assert norm_err(a.cpu().numpy(), r) <= TOL and norm_err(b.cpu().numpy(), r) <= TOL, n
        assert norm_err(b.cpu().numpy(), a.cpu().numpy()) <= TOL, n
    # the assembly's own gradients have a fixed order: the sources' repeat bit for bit
    for a, b in zip(first[4:len(leaves)], second[4:len(leaves)]):
        assert torch.equal(a, b)


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("kind", sorted(PARTS))
def test_module_autocast(kind, dt, monkeypatch):
    """The gradients of both routes under autocast against the fp32 module's
    on the same (dtype-rounded) inputs: the assembled route's error is at most
    1.25 times the unfused route's for every gradient, the project's factor
    (test_gru_backward_network_gpu.py::test_module_autocast)."""
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    monkeypatch.setattr(torch.backends.cudnn, "benchmark", False)
    m, args, assembled, plain, _ = case(kind)
    low = [t.to(dt) for t in args]
    if kind == "gru08":
        low[4] = low[4].float()             # the motion features stay fp32 under autocast
    ref = forward_backward(m, [t.float() for t in low], grad_out(), plain)
    g = grad_out(dt)

    def under_autocast(route):
        def run(mod, *a):
            with torch.autocast("cuda", dtype=dt):
                return route(mod, *a)
        return run

    unfused = forward_backward(m, low, g, under_autocast(plain))
    with Spies() as spies:
        fused = forward_backward(m, low, g, under_autocast(assembled))
    assert len(spies.backward) == 1 and len(spies.assemble) == 2
    bad = []
    for f, u, r, n in zip(fused, unfused, ref, names(kind)):
        assert f.dtype == u.dtype and f.shape == u.shape == r.shape, n
        e_f = norm_err(f.float().cpu().numpy(), r.cpu().numpy())
        e_u = norm_err(u.float().cpu().numpy(), r.cpu().numpy())
        print(f"{kind} {dt} {n}: norm_err vs fp32 assembled {e_f:.3e}, unfused {e_u:.3e}, ratio {e_f / e_u:.2f}")
        if n != "out" and not e_f <= 1.25 * e_u:
            bad.append((n, e_f, e_u))
    assert not bad, bad


@functools.lru_cache(maxsize=None)
def training_run(which):
    """(predictions, parameter gradients, the assemble_backward calls) of one
    training step at 64x96, 2 iterations, fp32, deterministic convolutions."""
    kw, cl = {"unfused": ({}, False), "assembled": (ALL, False), "without": (
        {k: v for k, v in ALL.items() if k != "fuse_gru_inputs_backward"}, False), "channels_last": (ALL, True)}[which]
    det = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        torch.manual_seed(0)
        model = RAFTStereo(StereoArgs(), **kw).eval().to(DEV)
        if cl:
            model = model.to(memory_format=torch.channels_last)
        with Spies() as spies:
            preds = model(*small_pair(), iters=2)
            preds[-1][:, 0].abs().mean().backward()
    finally:
        torch.backends.cudnn.deterministic = det
    grads = {n: p.grad.cpu() for n, p in model.named_parameters() if p.grad is not None}
    return [p.detach().cpu() for p in preds], grads, tuple(spies.backward)


def test_network_runs_the_adjoint_once_per_gru_call():
    assert len(training_run("assembled")[2]) == 6              # 3 GRUs x 2 iterations
    assert sorted(training_run("assembled")[2]) == [(4, 6)] * 2 + [(8, 12)] * 2 + [(16, 24)] * 2
    assert training_run("without")[2] == ()
    assert training_run("unfused")[2] == ()


def test_network_predictions_and_gradients():
    pu, gu, _ = training_run("unfused")
    pf, gf, _ = training_run("assembled")
    assert len(pf) == len(pu)
    for i, (p, q) in enumerate(zip(pf, pu)):
        mae = (p - q).abs().mean().item()
        print(f"iteration {i}: assembled vs unfused MAE {mae:.3e} px")
        assert mae <= MAE_PX, (i, mae)
    assert gf.keys() == gu.keys() and any("gru08.convq" in n for n in gf)
    for n in gu:
        assert gf[n].shape == gu[n].shape and gf[n].dtype == gu[n].dtype, n
        assert torch.isfinite(gf[n]).all(), n

    def flat(g):
        return np.concatenate([g[n].numpy().ravel() for n in gu])

    e_all = norm_err(flat(gf), flat(gu))
    print(f"all parameters concatenated: assembled vs unfused {e_all:.2e}")
    assert e_all <= TOL, e_all


def test_channels_last_network_keeps_gru08_on_the_old_route():
    """gru08's motion features are NCHW in a channels_last network
    (``_sources_fit``): no adjoint launch from it, one per call from the others."""
    _, grads, calls = training_run("channels_last")
    assert sorted(calls) == [(4, 6)] * 2 + [(8, 12)] * 2, calls
    assert grads.keys() == training_run("unfused")[1].keys()
    assert all(torch.isfinite(g).all() for g in grads.values())
