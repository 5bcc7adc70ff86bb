"""The fp16-pyramid lookup kernels (csrc/lookup_f16pyr.hip): every wrapper
exists, none has scratch or spilled registers, and each stays at four waves
per SIMD (<= 128 vector registers) like the bf16 instances it mirrors -- and
they are kernels of their own names, so the instance counts that other
resource tests take by mangled name are what they were.  CPU only: reads the
code object's metadata from the built .so (tools/kernel_resources.py)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from kernel_resources import kernels  # noqa: E402

LIB = os.path.join(ROOT, "raft-stereo_amd", "_build", "libraftcorr.so")


def _named(prefix):
    # _ZN2rc<len><name>I...: the template instances of exactly this kernel
    return [k for k in kernels(LIB) if k["name"].startswith(f"_ZN2rc{len(prefix)}{prefix}I")]


def _lean(k, sgpr_spill=0):
    # scratch / vgpr_spill: memory traffic per lane, never allowed
    # (test_kernel_resources.py); SGPR spills go to VGPR lanes, not memory
    assert not k["scratch"] and not k["vgpr_spill"], k
    assert k["sgpr_spill"] <= sgpr_spill, k
    assert k["vgpr"] + (k["agpr"] or 0) <= 128, k


def test_pair_wrappers():
    ks = _named("lookup_f16pyr_pair_kernel")
    # radius 1..4 x {2, 4} levels x {NCHW, channels-last} x {fp32, fp16, bf16} output
    assert len(ks) == 48, [k["name"] for k in ks]
    assert len({k["name"] for k in ks}) == 48
    for k in ks:
        _lean(k)
    # only the channels-last instances stage their output in LDS
    assert sum(1 for k in ks if k["lds"]) == 24


def test_per_level_wrappers():
    ks = {k["name"]: k for k in _named("lookup_f16pyr_level_kernel")}
    assert len(ks) == 8, sorted(ks)                         # radius 1..8
    twins = {k["name"]: k for k in kernels(LIB)}
    for r in range(1, 9):
        k = ks[f"_ZN2rc26lookup_f16pyr_level_kernelILi{r}EEEvNS_10LookupArgsE"]
        # the bf16 instance it mirrors: lookup_kernel<R, 0, true, true, 256, 1>.  No SGPR spills up
        # to radius 4 (what the pair layout and the network use); the wider windows of radius 5..8
        # keep some scalars in VGPR lanes in the bf16 kernel, and no more than that here
        twin = twins[f"_ZN2rc13lookup_kernelILi{r}ELi0ELb1ELb1ELi256ELi1EEEvNS_10LookupArgsE"]
        _lean(k, sgpr_spill=0 if r <= 4 else twin["sgpr_spill"])
        assert k["vgpr"] <= twin["vgpr"], (k, twin)
        assert not k["lds"], k


def test_f16_build_and_pool_instances_exist_without_scratch():
    names = {k["name"]: k for k in kernels(LIB)}
    # the 16-bit build templates carry the element kind last: ...ELi2EEE = fp16
    ring = [k for n, k in names.items() if n.startswith("_ZN2rc22build_bf16_ring_kernelI") and "ELi2EEEv" in n]
    wave = [k for n, k in names.items() if n.startswith("_ZN2rc17build_bf16_kernelI") and "ELi2EEEv" in n]
    # ring: {2..5 waves, deferred} + {2, 3, 4 waves x 4, 5 fragments}, each with 3 / 5 fused levels
    assert len(ring) == 20, sorted(n for n in names if "build_bf16_ring" in n)
    assert len(wave) == 4                                   # fp16 / fp32 fmaps x aligned / not
    for k in ring + wave:
        assert not k["scratch"] and not k["vgpr_spill"], k
    assert "_ZN2rc11pool_kernelILi2EEEvPKvxPvxxi" in names


def test_pinned_instance_counts_are_unchanged():
    names = [k["name"] for k in kernels(LIB)]
    assert sum(n.startswith("_ZN2rc18lookup_pair_kernelI") for n in names) == 96
    assert len(_named("lookup_pair_conv_kernel")) == 48
    assert len(_named("lookup_pair_conv_grad_kernel")) == 16
    assert sum("lookup_conv_bwd_kernel" in n for n in names) == 24
    assert sum("lookup_pair_conv" in n for n in names) == 64
    new = [n for n in names if "f16pyr" in n]
    assert len(new) == 56
    for n in new:
        assert "lookup_pair_kernel" not in n and "lookup_pair_conv" not in n and "lookup_conv_bwd" not in n
