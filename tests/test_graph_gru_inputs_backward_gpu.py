"""rc_gru_assemble_backward and one training step of a ConvGRU with
``fuse_inputs_backward`` under graph capture and replay: the protocol of
graph_util.py (captured, replayed after the static inputs were refilled, the
eager call's bits every time)."""
import pytest
import torch

from graph_util import DEV, captured
from raft_stereo_amd import gru
from raft_stereo_amd.network import ConvGRU

pytestmark = pytest.mark.gpu
SEED_A, SEED_B = 101, 202
DT = {"fp32": torch.float32, "bf16": torch.bfloat16}
FORMATS = {"planar": torch.contiguous_format, "channels_last": torch.channels_last}
# test_gru_inputs_gpu.py CASES: (N, H, W), ((mode, C, h, w), ...)
ASSEMBLE = {"tiny": ((1, 3, 5), (("copy", 8, 3, 5), ("pool2x", 3, 5, 9), ("bilinear", 5, 2, 3))),
            "w6": ((1, 2, 6), (("copy", 2, 2, 6), ("pool2x", 2, 3, 11), ("bilinear", 2, 2, 2)))}
GRU = (1, 8, 3, 5)          # N, C, H, W of the state; x = pool2x of 5x9 and interp of 2x3


def both(make):
    return make(torch.Generator().manual_seed(SEED_A)), make(torch.Generator().manual_seed(SEED_B))


@pytest.mark.parametrize("two", [False, True], ids=["g", "g+g2"])
@pytest.mark.parametrize("fmt", sorted(FORMATS))
@pytest.mark.parametrize("dt", sorted(DT))
@pytest.mark.parametrize("case", sorted(ASSEMBLE))
def test_assemble_backward(case, dt, fmt, two):
    (N, H, W), parts = ASSEMBLE[case]
    dtype, mf = DT[dt], FORMATS[fmt]
    C = sum(p[1] for p in parts)
    meta = tuple((mode, (N, Ci, h, w), dtype) for mode, Ci, h, w in parts)

    def fn(g, *g2):
        return gru.assemble_backward(g, meta, g2=g2[0] if g2 else None, g2_from=parts[0][1])

    captured(fn, *both(lambda gen: [torch.randn(N, C, H, W, generator=gen).to(dtype).contiguous(memory_format=mf)
                                    for _ in range(2 if two else 1)]))


@pytest.mark.parametrize("fmt", sorted(FORMATS))
@pytest.mark.parametrize("dt", sorted(DT))
def test_module_training_step(dt, fmt, monkeypatch):
    """Forward and backward of one ConvGRU on the assembled training route:
    the new state and the gradients of every input and gate weight."""
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    monkeypatch.setattr(torch.backends.cudnn, "benchmark", False)
    N, C, H, W = GRU
    dtype, mf = DT[dt], FORMATS[fmt]
    calls = []
    inner = gru.assemble_backward
    monkeypatch.setattr(gru, "assemble_backward", lambda *a, **kw: calls.append(1) or inner(*a, **kw))

    def make():
        torch.manual_seed(3)
        m = ConvGRU(C, 2 * C).eval().to(DEV).to(dtype).to(memory_format=mf)
        m.fuse = m.fuse_backward = m.fuse_inputs = m.fuse_inputs_backward = True
        params = list(m.parameters())

        def step(h, cz, cr, cq, a, b, g_out):
            leaves = [t.detach().requires_grad_(True) for t in (h, cz, cr, cq, a, b)]
            with torch.enable_grad():
                out = m(*leaves[:4], gru.Pooled(leaves[4]), gru.Resized(leaves[5], (H, W)))
                grads = torch.autograd.grad(out, leaves + params, g_out)
            return [out.detach(), *grads]

        return step

    def inputs(gen):
        def t(*shape):
            return torch.randn(shape, generator=gen).to(dtype).contiguous(memory_format=mf)
        h = torch.tanh(t(N, C, H, W).float()).to(dtype)
        return [h, t(N, C, H, W), t(N, C, H, W), t(N, C, H, W), t(N, C, 5, 9), t(N, C, 2, 3), t(N, C, H, W)]

    captured(None, *both(inputs), make=make)
    assert len(calls) == 4          # two eager calls, the warm-up and the capture; the replays run no Python
