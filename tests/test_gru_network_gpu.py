"""The fused ConvGRU route (gru.conv_gru_forward, RAFTStereo(fuse_gru=True),
DESIGN.md §3.7) against the unfused one: per module, against the reference's
golden disparity, under mixed precision, combined with the other options, and
with gradients enabled, where it must step aside."""
import numpy as np
import pytest
import torch

from golden_util import GOLDEN, image_digest, load, manifest, norm_err, stereo_pair
from raft_stereo_amd import gru
from raft_stereo_amd.network import ConvGRU, RAFTStereo, StereoArgs

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-5          # the project's fp32 bound (TOL of test_pair_convc1_gpu.py)
MAE_PX = 0.01       # the project's disparity bar (test_network_gpu.py)
# x_list of the three GRUs of the default network: gru32 takes pool2x(net[1]);
# gru16 pool2x(net[0]) and interp(net[2]); gru08 the motion features (fp32
# under autocast: they carry the fp32 flow) and interp(net[1])
PARTS = {"gru32": (128,), "gru16": (128, 128), "gru08": (128, 128)}


@pytest.fixture
def counted(monkeypatch):
    """Counts the calls of gru.gru_gates (one per fused ConvGRU.forward)."""
    calls = []
    inner = gru.gru_gates

    def spy(*a, **kw):
        calls.append(1)
        return inner(*a, **kw)

    monkeypatch.setattr(gru, "gru_gates", spy)
    return calls


def module_case(kind, channels_last=False):
    torch.manual_seed(3)
    m = ConvGRU(128, sum(PARTS[kind])).eval().to(DEV)
    g = torch.Generator().manual_seed(11)
    shape = (2, 128, 9, 20)
    h = torch.tanh(torch.randn(shape, generator=g))
    ctx = [torch.randn(shape, generator=g) for _ in range(3)]
    xs = [torch.randn(2, c, 9, 20, generator=g) for c in PARTS[kind]]
    args = [t.to(DEV) for t in [h] + ctx + xs]
    if channels_last:
        m = m.to(memory_format=torch.channels_last)
        args = [t.contiguous(memory_format=torch.channels_last) for t in args]
    return m, args


@pytest.mark.parametrize("channels_last", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("kind", sorted(PARTS))
def test_module_fp32(kind, channels_last, counted):
    m, args = module_case(kind, channels_last)
    with torch.no_grad():
        want = m(*args)
        assert not counted
        assert gru.why_not_fusable(m, *args) is None
        keep = [t.clone() for t in args]
        got = gru.conv_gru_forward(m, *args)
        m.fuse = True
        via = m(*args)
    assert len(counted) == 2
    assert all(torch.equal(a, b) for a, b in zip(args, keep)), "an input was modified"
    assert got.shape == want.shape and got.dtype == want.dtype
    assert gru._classes(got) & gru._classes(args[0]), "the new state is not in h's layout"
    err = norm_err(got.cpu().numpy(), want.cpu().numpy())
    print(f"{kind} fp32: fused vs unfused norm_err {err:.2e}")
    assert err <= TOL, err
    assert norm_err(via.cpu().numpy(), want.cpu().numpy()) <= TOL


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("kind", sorted(PARTS))
def test_module_autocast(kind, dt, counted):
    """Both routes under autocast against the fp32 unfused module on the same
    (dtype-rounded) inputs.  The fused route rounds once per kernel where the
    unfused one rounds after every op, so its error is expected below the
    unfused one's; the factor 1.25 leaves room for another MIOpen solver on
    the stacked convolution."""
    m, args = module_case(kind)
    low = [t.to(dt) for t in args]
    if kind == "gru08":
        low[4] = low[4].float()             # the motion features stay fp32 under autocast
    with torch.no_grad():
        ref = m(*[t.float() for t in low])
        with torch.autocast("cuda", dtype=dt):
            unfused = m(*low)
            assert not counted
            assert gru.why_not_fusable(m, *low) is None
            m.fuse = True
            fused = m(*low)
    assert len(counted) == 1
    assert fused.dtype == unfused.dtype == dt
    e_f = norm_err(fused.float().cpu().numpy(), ref.cpu().numpy())
    e_u = norm_err(unfused.float().cpu().numpy(), ref.cpu().numpy())
    print(f"{kind} {dt}: norm_err vs fp32 fused {e_f:.3e}, unfused {e_u:.3e}, ratio {e_f / e_u:.2f}")
    assert e_f <= 1.25 * e_u, (e_f, e_u)


def test_golden_config1(counted):
    """RAFTStereo(fuse_gru=True) on BASELINE configs[0] (320x720, 12
    iterations) against the reference's final disparity."""
    case = manifest()["cases"]["e2e_config1"]
    z = load(f"{GOLDEN}/e2e_config1.npz")
    img1, img2 = stereo_pair(1, case["H"], case["W"], case["seed"])
    assert image_digest(img1, img2) == case["image_sha256"]
    torch.manual_seed(0)
    model = RAFTStereo(StereoArgs(**case["args"]), fuse_gru=True).eval().to(DEV)
    with torch.no_grad():
        flows = model(img1.to(DEV), img2.to(DEV), iters=case["iters"])
    assert len(counted) == 3 * case["iters"]
    disp = flows[-1][:, 0].cpu().numpy()
    mae = float(np.abs(disp - z["disparity"]).mean())
    print(f"e2e_config1 fuse_gru: final MAE {mae:.2e} px")
    assert mae <= MAE_PX, mae


def small_pair():
    g = torch.Generator().manual_seed(8)
    img1 = (torch.rand(1, 3, 64, 96, generator=g) * 255).to(DEV)
    return img1, torch.roll(img1, -4, dims=-1)


def predictions(args, iters=3, **kw):
    torch.manual_seed(0)
    model = RAFTStereo(args, **kw).eval().to(DEV)
    with torch.no_grad():
        return [p.float().cpu() for p in model(*small_pair(), iters=iters)]


def assert_close_px(got, base, what):
    assert len(got) == len(base)
    for i, (p, q) in enumerate(zip(got, base)):
        mae = (p - q).abs().mean().item()
        print(f"{what}, iteration {i}: MAE {mae:.3e} px")
        assert mae <= MAE_PX, (what, i, mae)


def test_mixed_precision(counted):
    """fp16 autocast (the default autocast dtype), as
    test_network_hands_convc2_the_autocast_dtype runs it."""
    args = StereoArgs(mixed_precision=True)
    base = predictions(args)
    assert not counted
    got = predictions(args, fuse_gru=True)
    assert len(counted) == 3 * 3                 # gru32, gru16, gru08 in each of 3 iterations
    assert_close_px(got, base, "mixed precision")


def test_with_fuse_step(counted):
    base = predictions(StereoArgs(), fuse_step=True)
    got = predictions(StereoArgs(), fuse_step=True, fuse_gru=True)
    assert len(counted) == 9
    assert_close_px(got, base, "fuse_step")


def test_two_layers_slow_fast(counted):
    args = StereoArgs(n_gru_layers=2, slow_fast_gru=True)
    base = predictions(args)
    got = predictions(args, fuse_gru=True)
    assert len(counted) == 3 * 3                 # gru16 alone, then gru16 and gru08, per iteration
    assert_close_px(got, base, "n_gru_layers=2, slow_fast_gru")


def test_gradients_take_the_torch_ops(counted, monkeypatch):
    """Grad mode, trainable weights: fuse_gru changes nothing -- the same ops
    run, so outputs and parameter gradients are the unfused network's bit for
    bit (deterministic convolution algorithms asked for, as a training run
    that compares runs would) -- and no kernel of gru.py is called."""
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    img1, img2 = small_pair()
    outs = []
    for fuse in (False, True):
        torch.manual_seed(0)
        model = RAFTStereo(StereoArgs(), fuse_gru=fuse).eval().to(DEV)
        preds = model(img1, img2, iters=2)
        preds[-1][:, 0].abs().mean().backward()
        outs.append(([p.detach().cpu() for p in preds],
                     {n: p.grad.cpu() for n, p in model.named_parameters() if p.grad is not None}))
    assert not counted
    (pa, ga), (pb, gb) = outs
    assert all(torch.equal(a, b) for a, b in zip(pa, pb))
    assert ga.keys() == gb.keys() and any("gru08.convq" in n for n in ga)
    bad = [n for n in ga if not torch.equal(ga[n], gb[n])]
    assert not bad, bad
