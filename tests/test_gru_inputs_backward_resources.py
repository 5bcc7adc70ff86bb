"""The adjoint of the ConvGRU input assembly (csrc/gru_inputs_bwd.hip): every
instance exists and none has scratch, spilled registers or LDS; the hard cap
is 128 vector registers (four waves per SIMD), and the figure the build
achieves, 62 (the interleaved 16-byte instances of the 16-bit types; every
other instance is at or under 49), is asserted so that a regression shows.
CPU only: reads the code object's metadata from the built .so
(tools/kernel_resources.py)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from kernel_resources import kernels  # noqa: E402

LIB = os.path.join(ROOT, "raft-stereo_amd", "_build", "libraftcorr.so")
NAME = "gru_assemble_bwd_kernel"
CAP = 128
ACHIEVED = 62


def test_instances():
    ks = [k for k in kernels(LIB) if k["name"].startswith(f"_ZN2rc{len(NAME)}{NAME}I")]
    # {fp32, fp16, bf16} x {16-byte, 8-byte, one-element} accesses x {planar, interleaved}
    assert len(ks) == 18, [k["name"] for k in ks]
    assert len({k["name"] for k in ks}) == 18
    for k in ks:
        assert not k["scratch"] and not k["vgpr_spill"] and not k["sgpr_spill"], k
        assert not k["lds"], k
        assert k["vgpr"] + (k["agpr"] or 0) <= CAP, k
    worst = max(k["vgpr"] + (k["agpr"] or 0) for k in ks)
    print(sorted((k["vgpr"] + (k["agpr"] or 0), k["name"]) for k in ks))
    assert worst <= ACHIEVED, worst
