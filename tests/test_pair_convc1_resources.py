"""The fused lookup + convc1 kernels on the pair layout
(csrc/lookup_pair_conv.hip): every instance exists, none has scratch or
spilled registers, the forward stays at four waves per SIMD (<= 128 vector
registers, like lookup_pair_kernel and the per-level lookup_conv_kernel) and
the backward keeps what lets two workgroups share a CU, from the argument of
test_convc1_backward_resources.py: at most 80 KB of LDS and at most 256
vector registers (VGPR + AGPR).  CPU only: reads the code object's metadata
from the built .so (tools/kernel_resources.py)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from kernel_resources import kernels  # noqa: E402

LIB = os.path.join(ROOT, "raft-stereo_amd", "_build", "libraftcorr.so")


def _named(prefix):
    # _ZN2rc<len><name>I...: the template instances of exactly this kernel
    return [k for k in kernels(LIB) if k["name"].startswith(f"_ZN2rc{len(prefix)}{prefix}I")]


def test_forward_instances_run_four_waves_per_simd():
    ks = _named("lookup_pair_conv_kernel")
    # radius 1..4 x {2, 4} levels x {fp32, bf16} pyramid x {fp32, fp16, bf16} output
    assert len(ks) == 48, [k["name"] for k in ks]
    for k in ks:
        assert not k["scratch"] and not k["vgpr_spill"] and not k["sgpr_spill"], k
        assert not k["lds"], k
        assert k["vgpr"] + (k["agpr"] or 0) <= 128, k


def test_backward_instances_fit_two_workgroups_per_cu():
    ks = _named("lookup_pair_conv_grad_kernel")
    # radius 1..4 x {2, 4} levels x {fp32, bf16} pyramid
    assert len(ks) == 16, [k["name"] for k in ks]
    for k in ks:
        assert not k["scratch"] and not k["vgpr_spill"], k
        assert k["lds"] <= 80 * 1024, k
        assert k["vgpr"] + (k["agpr"] or 0) <= 256, k


def test_existing_kernel_names_are_not_shadowed():
    """The counts other resource tests take by name stay what they were."""
    names = [k["name"] for k in kernels(LIB)]
    assert sum("lookup_conv_bwd_kernel" in n for n in names) == 24
    assert sum("lookup_conv_bwd_reduce_kernel" in n for n in names) == 1
    new = [n for n in names if "lookup_pair_conv" in n]
    assert len(new) == 64
    assert not any(n.startswith("_ZN2rc18lookup_pair_kernelI") for n in new)
