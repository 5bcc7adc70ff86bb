"""RAFTStereo.forward(test_mode=True) on the GPU against the routes it
replaces, on one model per configuration (64 x 96 images, 3 iterations,
deterministic convolution algorithms): flow_low is forward()'s last prediction
and flow_up is forward(upsample=True)'s, bit for bit -- the 0.25 * mask of
today's route is exact in half precision for logits of this size (a power of
two, no subnormals), so `0.25f * widen(mask)` inside rc_upsample_head gives
the fp32 values convex_upsample is handed there.  The mask head runs once, and
the C ABI sees exactly one rc_upsample_head and no rc_convex_upsample."""
import pytest
import torch

from raft_stereo_amd import _lib
from raft_stereo_amd.network import RAFTStereo, StereoArgs

pytestmark = pytest.mark.gpu
DEV = "cuda"
ITERS = 3
BF16, F16 = torch.bfloat16, torch.float16

# name -> (StereoArgs keywords, autocast dtype or None, model keywords, channels_last)
CONFIGS = {
    "default": ({}, None, {}, False),
    "fuse_convc1": ({}, None, {"fuse_convc1": True}, False),
    "fuse_step": ({}, None, {"fuse_step": True}, False),
    "fuse_gru_inputs": ({}, None, {"fuse_gru": True, "fuse_gru_inputs": True}, False),
    "two_layers_slow_fast": ({"n_gru_layers": 2, "slow_fast_gru": True}, None, {}, False),
    "bf16": ({"mixed_precision": True}, BF16, {}, False),
    "bf16_channels_last": ({"mixed_precision": True}, BF16, {}, True),
    "fp16_pyramid": ({"mixed_precision": True}, F16, {"corr_pyramid_dtype": "autocast"}, False),
}


@pytest.fixture
def pinned_convs(monkeypatch):
    """Deterministic convolution algorithms, as test_gru_inputs_network_gpu.py asks for them."""
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    monkeypatch.setattr(torch.backends.cudnn, "benchmark", False)


def small_pair():
    g = torch.Generator().manual_seed(8)
    img1 = (torch.rand(1, 3, 64, 96, generator=g) * 255).to(DEV)
    return img1, torch.roll(img1, -4, dims=-1)


class Names:
    """Stands in for the CDLL (the ``_lib._active`` hook): forwards everything
    and keeps the names of the rc_* entry points called."""

    def __init__(self, real):
        self._real = real
        self.names = []

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if name in _lib.SIGNATURES and name not in ("rc_abi_version", "rc_last_error"):
            self.names.append(name)
        return fn


def bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


@pytest.mark.parametrize("name", list(CONFIGS))
def test_test_mode(name, pinned_convs):
    a, auto, kw, cl = CONFIGS[name]
    args = StereoArgs(**a)
    if auto is not None:
        args.autocast_dtype = auto
    torch.manual_seed(0)
    model = RAFTStereo(args, **kw).eval().to(DEV)
    if cl:
        model = model.to(memory_format=torch.channels_last)
    img1, img2 = small_pair()
    calls = []
    hook = model.update_block.mask[0].register_forward_hook(lambda m, i, o: calls.append(o.dtype))
    with torch.no_grad():
        low = model(img1, img2, iters=ITERS)
        assert len(calls) == ITERS
        up = model(img1, img2, iters=ITERS, upsample=True)
        del calls[:]
        rec = Names(_lib.lib())
        prev, _lib._active = _lib._active, rec
        try:
            out = model(img1, img2, iters=ITERS, test_mode=True)
            torch.cuda.synchronize()
        finally:
            _lib._active = prev
    hook.remove()
    assert isinstance(out, tuple) and len(out) == 2
    flow_low, flow_up = out
    assert len(calls) == 1
    if auto is not None:
        assert calls[0] == auto                      # the head read the mask in the autocast dtype
    assert rec.names.count("rc_upsample_head") == 1 and "rc_convex_upsample" not in rec.names
    assert flow_low.dtype == torch.float32 and tuple(flow_low.shape) == (1, 2, 16, 24)
    assert flow_up.dtype == torch.float32 and tuple(flow_up.shape) == (1, 1, 64, 96)
    assert torch.equal(bits(flow_low), bits(low[-1])), name
    assert float(up[-1].abs().max()) > 0
    diff = int((bits(flow_up) != bits(up[-1])).sum())
    assert not diff, f"{name}: {diff} of {flow_up.numel()} elements of flow_up differ from forward(upsample=True)[-1]"


def test_refusals():
    torch.manual_seed(0)
    model = RAFTStereo(StereoArgs()).eval().to(DEV)
    img1, img2 = small_pair()
    with torch.no_grad(), pytest.raises(ValueError, match="iters"):
        model(img1, img2, iters=0, test_mode=True)
    with torch.enable_grad(), pytest.raises(RuntimeError, match="inference-only"):
        model(img1, img2, iters=1, test_mode=True)
