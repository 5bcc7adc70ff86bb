"""RAFTStereo.forward as a graph replay ("Graph capture";
DESIGN.md §6): a 64x96 pair, 3 iterations, eval mode, no gradient.  Three
eager forwards come first, so the convolution library settles its algorithms
outside the capture; then one forward is captured on static images and goes
through the protocol of graph_util.captured -- images A, refilled with B,
then A again -- against eager forwards on fresh tensors.

The project's kernels are bit-reproducible; the convolutions are PyTorch's,
run with deterministic algorithms asked for (as
test_gru_inputs_network_gpu.py does).  EAGER_NOISE holds, per variant, the
largest norm_err between two eager forwards of the same model on the same
images (``eager_noise`` below measures it: four forwards per image pair, two
pairs).  Where it is 0 the replay must equal the eager forward bit for bit.
Where it is not, an fp32 variant is held to norm_err <= 1e-5, the project's
fp32 bound (TOL of test_gru_network_gpu.py), and the bf16 variant to twice its
measured figure, as test_gru_backward_gpu.py allows twice its measured ratios.
Measured on an MI355X: 0 for all six variants, so every one of
them is held to bit equality.
"""
import pytest
import torch

from golden_util import norm_err
from graph_util import DEV, bits, captured, eager, same_bits, within
from raft_stereo_amd.network import RAFTStereo, StereoArgs

pytestmark = pytest.mark.gpu
TOL = 1e-5          # the project's fp32 bound (test_gru_network_gpu.py)
ITERS = 3

# name: (StereoArgs keywords, autocast dtype, RAFTStereo keywords, channels_last, forward keywords)
VARIANTS = {
    "default": ({}, None, {}, False, {}),
    "fuse_step": ({}, None, {"fuse_step": True}, False, {}),
    "fuse_convc1": ({}, None, {"fuse_convc1": True}, False, {}),
    "fuse_gru_inputs": ({}, None, {"fuse_gru": True, "fuse_gru_inputs": True}, False, {}),
    "bf16_channels_last": ({"mixed_precision": True}, torch.bfloat16,
                           {"corr_out_dtype": "autocast", "fuse_gru": True, "fuse_gru_inputs": True}, True, {}),
    "upsample": ({}, None, {}, False, {"upsample": True}),
}

# largest eager-against-eager norm_err over the predictions; 0.0: bit-stable
EAGER_NOISE = {
    "default": 0.0,
    "fuse_step": 0.0,
    "fuse_convc1": 0.0,
    "fuse_gru_inputs": 0.0,
    "bf16_channels_last": 0.0,
    "upsample": 0.0,
}


@pytest.fixture(autouse=True)
def pinned(monkeypatch):
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    monkeypatch.setattr(torch.backends.cudnn, "benchmark", False)
    with torch.no_grad():
        yield


def images(seed):
    g = torch.Generator().manual_seed(seed)
    img1 = torch.rand(1, 3, 64, 96, generator=g) * 255
    return [img1, torch.roll(img1, -4, dims=-1)]


def network(name):
    """The variant's model and its forward as a function of the two images."""
    a, autocast, kw, channels_last, fkw = VARIANTS[name]
    args = StereoArgs(**a)
    if autocast is not None:
        args.autocast_dtype = autocast
    torch.manual_seed(0)
    model = RAFTStereo(args, **kw).eval().to(DEV)
    if channels_last:
        model = model.to(memory_format=torch.channels_last)
    return model, lambda img1, img2: channels(model(img1, img2, iters=ITERS, **fkw))


def channels(predictions):
    """Each low-resolution prediction as its x-flow and its y-flow, two views
    of the one tensor: the network zeroes the y-flow of every iteration
    (network.py, the D8 tail), so that half is the same whatever the images
    show, and the discrimination condition is judged on the x-flows.  The
    upsampled predictions are x-flow only."""
    return [p[:, k:k + 1] for p in predictions for k in range(p.shape[1])]


def y_flows(name):
    return () if VARIANTS[name][4].get("upsample") else tuple(range(1, 2 * ITERS, 2))


def comparison(name):
    noise = EAGER_NOISE[name]
    if noise == 0.0:
        return same_bits
    return within(2 * noise if VARIANTS[name][1] is not None else TOL)


def eager_noise(name, runs=4):
    """The largest norm_err between two of ``runs`` eager forwards, over both
    image pairs and every prediction (what EAGER_NOISE records)."""
    _, forward = network(name)
    worst = 0.0
    for seed in (8, 9):
        outs = [eager(forward, images(seed))[0] for _ in range(runs)]
        for i in range(runs):
            for j in range(i + 1, runs):
                for p, q in zip(outs[i], outs[j]):
                    worst = max(worst, norm_err(p.view(torch.float32).numpy(), q.view(torch.float32).numpy()))
    return worst


@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_forward_as_a_replay(name):
    _, forward = network(name)
    want_a, _ = captured(forward, images(8), images(9), warmups=3, compare=comparison(name), constant=y_flows(name))
    assert len(want_a) == ITERS * (1 if VARIANTS[name][4].get("upsample") else 2)


def perturbed(state, seed):
    g = torch.Generator().manual_seed(seed)
    return {k: v * (1 + 0.05 * torch.randn(v.shape, generator=g)).to(v.device, v.dtype) if v.is_floating_point()
            else v for k, v in state.items()}


def test_new_weights_need_a_new_capture():
    """fuse_gru stacks the z and r gate weights into a cached copy (gru._ZR):
    after load_state_dict a second capture restacks them -- the cache entry is
    then created inside the capture -- and its replay equals the eager
    forward with the new weights, which afterwards reads that same entry."""
    name = "fuse_gru_inputs"
    model, forward = network(name)
    compare = comparison(name)
    static = [t.to(DEV) for t in images(8)]

    def capture():
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            outs = forward(*static)
        graph.replay()
        torch.cuda.synchronize()
        return graph, [bits(t) for t in outs]

    for _ in range(3):
        forward(*static)
    torch.cuda.synchronize()
    old_eager = eager(forward, images(8))[0]
    graph1, old = capture()
    compare(old, old_eager, "replay with the first weights")

    model.load_state_dict(perturbed(model.state_dict(), 5))
    graph2, new = capture()
    new_eager = eager(forward, images(8))[0]
    compare(new, new_eager, "replay of the second capture against the eager forward with the new weights")
    x = [i for i in range(len(new_eager)) if i not in y_flows(name)]
    changed = sum(int((new_eager[i] != old_eager[i]).sum()) for i in x) / sum(new_eager[i].numel() for i in x)
    assert changed > 0.5, f"vacuous: the new weights changed {changed:.3f} of the predictions only"
