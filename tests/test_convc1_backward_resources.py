"""The backward kernels of the fused lookup + convc1 (csrc/lookup_conv_bwd.hip)
must keep what lets two workgroups share a CU: at most 80 KB of LDS
(2 x 80 KB = the CU's 160 KB), at most 256 vector registers (VGPR + AGPR: two
256-thread workgroups put two waves on each SIMD, 512 / 2 per lane), no
scratch and no VGPR spills -- for all 24 instances (radius 1..4, levels 2..4,
fp32 and bf16 pyramid).  CPU only: reads the code object's metadata from the
built .so (tools/kernel_resources.py)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from kernel_resources import kernels  # noqa: E402

LIB = os.path.join(ROOT, "raft-stereo_amd", "_build", "libraftcorr.so")


@pytest.mark.skipif(not os.path.exists(LIB), reason="libraftcorr.so not built")
def test_conv_bwd_kernels_fit_two_workgroups_per_cu():
    ks = [k for k in kernels(LIB) if "lookup_conv_bwd_kernel" in k["name"]]
    assert len(ks) == 24, [k["name"] for k in ks]
    for k in ks:
        assert k["lds"] <= 80 * 1024, k
        assert k["vgpr"] + (k["agpr"] or 0) <= 256, k
        assert not k["scratch"] and not k["vgpr_spill"], k
    red = [k for k in kernels(LIB) if "lookup_conv_bwd_reduce_kernel" in k["name"]]
    assert len(red) == 1 and not red[0]["scratch"] and not red[0]["vgpr_spill"]
