"""Resources of the compound prediction kernels (CPU test, no GPU), read from the code object in the library's build
objects as test_kernel_resources_small.py does.  compound_kernel (the batch: 256 lanes, four waves with a private LDS
slice each) and jnt_block_kernel (the shims: one wave) exist for both sample types and keep everything in registers: the
first reference's CONV_BUF_TYPE values live in a lane's registers between the two passes, so scratch there would be the
intermediate in memory after all."""
import os
import shutil
import tempfile

import pytest

from test_kernel_resources import BUILD, LLVM
from test_kernel_resources_small import _meta

WAVE_LDS = (2112 + 1248) * 2  # kWinCap + kImCap 16-bit elements


@pytest.fixture(scope="module")
def kernels():
    obj = os.path.join(BUILD, "compound.o")
    if not os.path.exists(obj) or not os.path.exists(os.path.join(LLVM, "clang-offload-bundler")):
        pytest.skip("needs the built objects and the ROCm LLVM tools")
    tmp = tempfile.mkdtemp()
    try:
        return _meta(obj, tmp)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


@pytest.mark.parametrize("name,lds", [("compound_kernel", 4 * WAVE_LDS), ("jnt_block_kernel", WAVE_LDS)])
def test_instances_for_both_sample_types_without_scratch_or_spills(kernels, name, lds):
    mine = {n: m for n, m in kernels.items() if name in n}
    assert len(mine) == 2 and any("IhE" in n for n in mine) and any("ItE" in n for n in mine), sorted(kernels)
    for n, m in mine.items():
        assert m.get("private_segment_fixed_size", 0) == 0, (n, m)
        assert m.get("vgpr_spill_count", 0) == 0 and m.get("sgpr_spill_count", 0) == 0, (n, m)
        assert m["group_segment_fixed_size"] == lds, (n, m)


def test_no_other_kernels_in_the_object(kernels):
    assert all("compound_kernel" in n or "jnt_block_kernel" in n for n in kernels), sorted(kernels)
