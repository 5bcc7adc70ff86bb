"""The backward kernels of the ConvGRU glue (csrc/gru_gates_bwd.hip): every
instance exists, none has scratch, spilled registers or LDS, and all stay at or
under 64 vector registers (eight waves per SIMD), the forward kernels' limits;
and the forward kernels keep their nine instances each.  CPU only: reads the
code object's metadata from the built .so (tools/kernel_resources.py)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from kernel_resources import kernels  # noqa: E402

LIB = os.path.join(ROOT, "raft-stereo_amd", "_build", "libraftcorr.so")


def instances(name):
    return [k for k in kernels(LIB) if k["name"].startswith(f"_ZN2rc{len(name)}{name}I")]


@pytest.mark.parametrize("name", ["gru_gates_bwd_kernel", "gru_blend_bwd_kernel"])
def test_instances(name):
    ks = instances(name)
    # {fp32, fp16, bf16} x {16-byte, 8-byte, one-element} accesses
    assert len(ks) == 9, [k["name"] for k in ks]
    for k in ks:
        assert not k["scratch"] and not k["vgpr_spill"] and not k["sgpr_spill"], k
        assert not k["lds"], k
        assert k["vgpr"] + (k["agpr"] or 0) <= 64, k


@pytest.mark.parametrize("name", ["gru_gates_kernel", "gru_blend_kernel"])
def test_forward_instances_unchanged(name):
    ks = instances(name)
    assert len(ks) == 9, [k["name"] for k in ks]
    assert all("GruBwdArgs" not in k["name"] for k in ks)
