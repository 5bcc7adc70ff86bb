"""The instances of upsample_head_kernel in the built product library
(tools/kernel_resources.py; no GPU): all 3 element kinds x 2 layout classes x
4 factors x 2 access widths are there, none uses scratch, spills or LDS, and
the planar 8-byte instances of f = 8 -- which hold the packed logits of four
sub-pixels and one pixel's weights at a time -- stay within the 256 registers
a 512-lane workgroup leaves a lane."""
import os
import sys

import pytest

from raft_stereo_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from kernel_resources import kernels  # noqa: E402

KINDS = (_lib.RC_F32, _lib.RC_BF16, _lib.RC_F16)
FACTORS = (1, 2, 4, 8)


def mangled(ek, f, inter, wide):
    """upsample_head_kernel<EK, F, INTER, WIDE>(rc::HeadArgs), Itanium ABI."""
    return f"_ZN2rc20upsample_head_kernelILi{ek}ELi{f}ELb{int(inter)}ELb{int(wide)}EEEvNS_8HeadArgsE"


@pytest.fixture(scope="module")
def head_kernels():
    ks = {k["name"]: k for k in kernels(_lib.LIB_PATH) if "upsample_head_kernel" in k["name"]}
    assert ks, "no upsample_head_kernel instance in the product library"
    return ks


def test_every_instance_exists(head_kernels):
    want = {mangled(ek, f, inter, wide) for ek in KINDS for f in FACTORS for inter in (False, True)
            for wide in (False, True)}
    assert len(want) == 48
    assert set(head_kernels) == want


def test_no_scratch_no_spills_no_lds(head_kernels):
    bad = [(n, k["scratch"], k["vgpr_spill"], k["lds"]) for n, k in head_kernels.items()
           if k["scratch"] or k["vgpr_spill"] or k["lds"]]
    assert not bad, bad


def test_registers_fit_the_workgroup(head_kernels):
    """A workgroup of 64 f lanes is f waves, f / 4 per SIMD: 512 registers per
    lane up to f = 4, 256 at f = 8."""
    for ek in KINDS:
        for f in FACTORS:
            for inter in (False, True):
                for wide in (False, True):
                    k = head_kernels[mangled(ek, f, inter, wide)]
                    assert k["vgpr"] + (k["agpr"] or 0) <= (256 if f == 8 else 512), (ek, f, inter, wide, k)
