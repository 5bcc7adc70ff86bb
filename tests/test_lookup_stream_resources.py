"""Every lookup_pair_kernel instance of the product library (csrc/lookup_pair.h)
keeps what its pinned load schedule is built around: at most 128 vector
registers (four waves per SIMD: the whole sceneflow grid, 4,050 waves, is
resident in one round), no scratch and no VGPR spills.  CPU only: reads the
code object's metadata from the built .so (tools/kernel_resources.py)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from kernel_resources import kernels  # noqa: E402

LIB = os.path.join(ROOT, "raft-stereo_amd", "_build", "libraftcorr.so")
PAIR = "_ZN2rc18lookup_pair_kernelI"
# radius 1..4 x 2 / 4 levels x fp32 / bf16 pyramid x NCHW / channels-last, for
# the fp32 output (lookup.hip) and the fp16 / bf16 outputs (lookup_half.hip)
INSTANCES = 4 * 2 * 2 * 2 * 3


@pytest.mark.skipif(not os.path.exists(LIB), reason="libraftcorr.so not built")
def test_pair_kernels_keep_four_waves_per_simd():
    hit = [k for k in kernels(LIB) if k["name"].startswith(PAIR)]
    assert len(hit) == INSTANCES, f"{len(hit)} lookup_pair_kernel instances in the product library"
    for k in hit:
        print(k["name"], k["vgpr"], k["agpr"], k["scratch"], k["vgpr_spill"])
        assert k["vgpr"] + (k["agpr"] or 0) <= 128, k
        assert not k["scratch"] and not k["vgpr_spill"], k
