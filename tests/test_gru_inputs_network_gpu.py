"""The assembled ConvGRU inputs (gru.assemble, ConvGRU.fuse_inputs,
RAFTStereo(fuse_gru_inputs=True)) against the routes that
compute pool2x / interp / cat with the PyTorch ops: per module, against the
reference's golden disparity, under mixed precision, combined with the other
options, and with gradients enabled, where it must step aside."""
import numpy as np
import pytest
import torch

from golden_util import GOLDEN, image_digest, load, manifest, norm_err, stereo_pair
from raft_stereo_amd import gru, network
from raft_stereo_amd.network import ConvGRU, RAFTStereo, StereoArgs

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-5          # the project's fp32 bound (test_gru_network_gpu.py)
MAE_PX = 0.01       # the project's disparity bar (test_gru_network_gpu.py)
# x_list of the three GRUs of the default network: gru32 takes pool2x(net[1]);
# gru16 pool2x(net[0]) and interp(net[2]); gru08 the motion features (fp32
# under autocast: they carry the fp32 flow) and interp(net[1])
PARTS = {"gru32": ("pool",), "gru16": ("pool", "resize"), "gru08": ("plain", "resize")}
H_SHAPE, POOL_SRC, RESIZE_SRC = (2, 128, 9, 20), (2, 128, 17, 39), (2, 128, 5, 10)


@pytest.fixture
def counted(monkeypatch):
    """Counts the calls of gru.assemble, network.pool2x and network.interp."""
    calls = {"assemble": 0, "pool2x": 0, "interp": 0}

    def spy(mod, name):
        inner = getattr(mod, name)

        def wrapped(*a, **kw):
            calls[name] += 1
            return inner(*a, **kw)

        monkeypatch.setattr(mod, name, wrapped)

    spy(gru, "assemble")
    spy(network, "pool2x")
    spy(network, "interp")
    return calls


def module_case(kind, channels_last=False):
    """(module, h + context, the sources of x, a function from sources to the
    lazy x_list)."""
    torch.manual_seed(3)
    m = ConvGRU(128, 128 * len(PARTS[kind])).eval().to(DEV)
    g = torch.Generator().manual_seed(11)
    h = torch.tanh(torch.randn(H_SHAPE, generator=g))
    ctx = [torch.randn(H_SHAPE, generator=g) for _ in range(3)]
    shapes = {"pool": POOL_SRC, "resize": RESIZE_SRC, "plain": H_SHAPE}
    srcs = [torch.randn(shapes[p], generator=g) for p in PARTS[kind]]
    state = [t.to(DEV) for t in [h] + ctx]
    srcs = [t.to(DEV) for t in srcs]
    if channels_last:
        m = m.to(memory_format=torch.channels_last)
        state = [t.contiguous(memory_format=torch.channels_last) for t in state]
        srcs = [t.contiguous(memory_format=torch.channels_last) for t in srcs]

    def lazy(srcs):
        make = {"pool": gru.Pooled, "resize": lambda t: gru.Resized(t, H_SHAPE[2:]), "plain": lambda t: t}
        return [make[p](t) for p, t in zip(PARTS[kind], srcs)]

    return m, state, srcs, lazy


@pytest.mark.parametrize("channels_last", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("kind", sorted(PARTS))
def test_module_fp32(kind, channels_last, counted):
    m, state, srcs, lazy = module_case(kind, channels_last)
    with torch.no_grad():
        want = m(*state, *gru.materialized(lazy(srcs)))          # the unfused module on materialised inputs
        assert not counted["assemble"]
        keep = [t.clone() for t in state + srcs]
        m.fuse = m.fuse_inputs = True
        assert gru.why_not_fusable(m, *state, *lazy(srcs)) is None
        got = m(*state, *lazy(srcs))
    assert counted["assemble"] == 1
    assert all(torch.equal(a, b) for a, b in zip(state + srcs, keep)), "an input was modified"
    assert got.shape == want.shape and got.dtype == want.dtype
    err = norm_err(got.cpu().numpy(), want.cpu().numpy())
    print(f"{kind} fp32: assembled + fused vs unfused norm_err {err:.2e}")
    assert err <= TOL, err


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("kind", sorted(PARTS))
def test_module_autocast(kind, dt, counted, monkeypatch):
    """Both routes under autocast against the fp32 unfused module on the same
    (dtype-rounded) inputs: the assembled route rounds the pooled and resized
    parts once where the torch ops round them and the concatenation copies
    them, so its error is expected at or below the unfused one's; the factor
    1.25 is test_gru_network_gpu.test_module_autocast's.  The statistic is a
    maximum over 46080 outputs a few ulps of the state wide, so the
    convolutions' algorithms are pinned (deterministic ones asked for, as
    test_gradients_leave_the_inputs_to_the_torch_ops does): without that the
    unfused route's own figure moves from run to run."""
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    monkeypatch.setattr(torch.backends.cudnn, "benchmark", False)
    m, state, srcs, lazy = module_case(kind)
    state = [t.to(dt) for t in state]
    srcs = [t.to(dt) for t in srcs]
    if kind == "gru08":
        srcs[0] = srcs[0].float()             # the motion features stay fp32 under autocast
    with torch.no_grad():
        ref = m(*[t.float() for t in state], *gru.materialized(lazy([t.float() for t in srcs])))
        with torch.autocast("cuda", dtype=dt):
            unfused = m(*state, *gru.materialized(lazy(srcs)))
            assert not counted["assemble"]
            m.fuse = m.fuse_inputs = True
            assert gru.why_not_fusable(m, *state, *lazy(srcs)) is None
            fused = m(*state, *lazy(srcs))
    assert counted["assemble"] == 1
    assert fused.dtype == unfused.dtype == dt
    e_f = norm_err(fused.float().cpu().numpy(), ref.cpu().numpy())
    e_u = norm_err(unfused.float().cpu().numpy(), ref.cpu().numpy())
    print(f"{kind} {dt}: norm_err vs fp32 assembled {e_f:.3e}, unfused {e_u:.3e}, ratio {e_f / e_u:.2f}")
    assert e_f <= 1.25 * e_u, (e_f, e_u)


ULP = {torch.float16: 2.0 ** -10, torch.bfloat16: 2.0 ** -7}


@pytest.mark.parametrize("channels_last", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("kind", sorted(PARTS))
def test_buffer_against_cat_of_the_materialised_parts(kind, dt, channels_last):
    """The assembled [h, x] buffer against ``torch.cat(out=)`` of the parts the
    PyTorch ops compute, element by element.  Both sides evaluate the same
    expression in fp32 on the same 16-bit inputs and round once to ``dt``;
    the fp32 values differ by a few fp32 ulps at most (another order of the
    same operations, a contracted multiply-add), so the rounded ones are
    equal or neighbours: |a - b| <= one ulp of the larger, 2^-10 (fp16) or
    2^-7 (bf16) of its magnitude.  h and the plain part are copies: equal."""
    m, state, srcs, lazy = module_case(kind, channels_last)
    h = state[0].to(dt)
    srcs = [t.to(dt) for t in srcs]
    if kind == "gru08":
        srcs[0] = srcs[0].float()
    fmt = torch.channels_last if channels_last else torch.contiguous_format
    with torch.no_grad():
        want = torch.empty((2, 128 * (1 + len(srcs)), 9, 20), dtype=dt, device=DEV, memory_format=fmt)
        torch.cat([h, *gru.materialized(lazy(srcs))], dim=1, out=want)
        got = gru.assemble([h, *lazy(srcs)], dt, fmt)
    assert got.shape == want.shape and got.dtype == dt and got.stride() == want.stride()
    a, b = got.float(), want.float()
    differ = int((a != b).sum())
    print(f"{kind} {dt}: {differ} of {a.numel()} elements differ from torch.cat's")
    assert torch.equal(a[:, :128], b[:, :128]), "h"
    if kind == "gru08":
        assert torch.equal(a[:, 128:256], b[:, 128:256]), "the cast motion features"
    # below the normal range the spacing is the smallest subnormal's
    floor = 2.0 ** -24 if dt == torch.float16 else 2.0 ** -133
    assert bool(((a - b).abs() <= (ULP[dt] * torch.maximum(a.abs(), b.abs())).clamp_min(floor)).all())


def test_golden_config1(counted):
    """RAFTStereo(fuse_gru=True, fuse_gru_inputs=True) on BASELINE configs[0]
    (320x720, 12 iterations) against the reference's final disparity."""
    case = manifest()["cases"]["e2e_config1"]
    z = load(f"{GOLDEN}/e2e_config1.npz")
    img1, img2 = stereo_pair(1, case["H"], case["W"], case["seed"])
    assert image_digest(img1, img2) == case["image_sha256"]
    torch.manual_seed(0)
    model = RAFTStereo(StereoArgs(**case["args"]), fuse_gru=True, fuse_gru_inputs=True).eval().to(DEV)
    with torch.no_grad():
        flows = model(img1.to(DEV), img2.to(DEV), iters=case["iters"])
    assert counted["assemble"] == 3 * case["iters"]
    assert counted["pool2x"] == 0 and counted["interp"] == 0
    disp = flows[-1][:, 0].cpu().numpy()
    mae = float(np.abs(disp - z["disparity"]).mean())
    print(f"e2e_config1 fuse_gru_inputs: final MAE {mae:.2e} px")
    assert mae <= MAE_PX, mae


def small_pair():
    g = torch.Generator().manual_seed(8)
    img1 = (torch.rand(1, 3, 64, 96, generator=g) * 255).to(DEV)
    return img1, torch.roll(img1, -4, dims=-1)


def predictions(args, iters=3, channels_last=False, **kw):
    torch.manual_seed(0)
    model = RAFTStereo(args, **kw).eval().to(DEV)
    if channels_last:
        model = model.to(memory_format=torch.channels_last)
    with torch.no_grad():
        return [p.float().cpu() for p in model(*small_pair(), iters=iters)]


def assert_close_px(got, base, what):
    assert len(got) == len(base)
    for i, (p, q) in enumerate(zip(got, base)):
        mae = (p - q).abs().mean().item()
        print(f"{what}, iteration {i}: MAE {mae:.3e} px")
        assert mae <= MAE_PX, (what, i, mae)


# (StereoArgs keywords, model keywords, assemble calls per iteration); the GRUs
# that are not assembled materialise their descriptors: one interp call per
# iteration for gru08
OPTIONS = {
    "fp16": ({"mixed_precision": True}, {}, 3),
    "fuse_step": ({}, {"fuse_step": True}, 3),
    "two_layers_slow_fast": ({"n_gru_layers": 2, "slow_fast_gru": True}, {}, 3),   # gru16, then gru16 and gru08
    "one_layer": ({"n_gru_layers": 1}, {}, 1),                                    # gru08 with the motion part only
    # gru32 and gru16; gru08's motion features are NCHW (concatenated with the flow), so it keeps the torch ops
    "channels_last": ({}, {"channels_last": True}, 2),
}


@pytest.mark.parametrize("option", sorted(OPTIONS))
def test_against_fuse_gru_alone(option, counted):
    a, kw, per_iter = OPTIONS[option]
    base = predictions(StereoArgs(**a), fuse_gru=True, **kw)
    assert not counted["assemble"]
    before = dict(counted)
    got = predictions(StereoArgs(**a), fuse_gru=True, fuse_gru_inputs=True, **kw)
    assert counted["assemble"] == per_iter * 3
    left = 3 if option == "channels_last" else 0          # gru08's interp, once per iteration
    assert counted["pool2x"] == before["pool2x"] and counted["interp"] == before["interp"] + left
    assert_close_px(got, base, option)


@pytest.mark.parametrize("backward", [False, True], ids=["torch_ops", "fuse_gru_backward"])
def test_gradients_leave_the_inputs_to_the_torch_ops(backward, counted, monkeypatch):
    """Grad mode, trainable weights: fuse_gru_inputs changes nothing -- the
    descriptors are materialised by the same ops before anything else, so
    predictions and parameter gradients are bit for bit those of the same
    model without it (deterministic algorithms asked for, as
    test_gru_network_gpu.test_gradients_take_the_torch_ops does) -- and
    gru.assemble is never called."""
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    img1, img2 = small_pair()
    outs = []
    for inputs in (False, True):
        torch.manual_seed(0)
        model = RAFTStereo(StereoArgs(), fuse_gru=True, fuse_gru_backward=backward,
                           fuse_gru_inputs=inputs).eval().to(DEV)
        preds = model(img1, img2, iters=2)
        preds[-1][:, 0].abs().mean().backward()
        outs.append(([p.detach().cpu() for p in preds],
                     {n: p.grad.cpu() for n, p in model.named_parameters() if p.grad is not None}))
    assert not counted["assemble"]
    (pa, ga), (pb, gb) = outs
    assert all(torch.equal(a, b) for a, b in zip(pa, pb))
    assert ga.keys() == gb.keys() and any("gru08.convq" in n for n in ga)
    bad = [n for n in ga if not torch.equal(ga[n], gb[n])]
    assert not bad, bad
