"""The three-slot split-bf16 build kernels (csrc/volume_split.hip,
build_split_kernel<.., 128, 3>) must keep what lets three workgroups share a
CU: at most 53,248 B of LDS (3 x 53,248 <= 160 KB), at most 168 vector
registers (VGPR + AGPR: 512 / 3 per SIMD lane in steps of 8), no scratch and
no VGPR spills.  CPU only: reads the code object's metadata from the built
.so (tools/kernel_resources.py)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from kernel_resources import kernels  # noqa: E402

LIB = os.path.join(ROOT, "raft-stereo_amd", "_build", "libraftcorr.so")
# build_split_kernel<MODE = 0, NLM, TW = 128, SL = 3>: the 3- and the 5-level instance
RING3 = ["_ZN2rc18build_split_kernelILi0ELi3ELi128ELi3EEE", "_ZN2rc18build_split_kernelILi0ELi5ELi128ELi3EEE"]


@pytest.mark.skipif(not os.path.exists(LIB), reason="libraftcorr.so not built")
def test_ring3_kernels_fit_three_workgroups_per_cu():
    ks = {k["name"]: k for k in kernels(LIB)}
    for prefix in RING3:
        hit = [k for n, k in ks.items() if n.startswith(prefix)]
        assert len(hit) == 1, f"{prefix}: not in the product library"
        k = hit[0]
        print(k)
        assert k["lds"] <= 53248, k
        assert k["vgpr"] + (k["agpr"] or 0) <= 168, k
        assert not k["scratch"] and not k["vgpr_spill"], k
