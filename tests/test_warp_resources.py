"""Resources of the warped-motion kernels (CPU test, no GPU), read from the code object in the library's build objects as
test_masked_compound_resources.py does.  warp_kernel (the batch) and warp_block_kernel (the two shims) exist once per
sample type and nothing else is in the object.  A workgroup's LDS is the filter table (193 rows of 16 bytes) and four
waves' private slices (a 15 x 16 patch and the 15 x 8 horizontal results, 16 bits each); a compound block's first
CONV_BUF_TYPE value stays in a register, so scratch would be the intermediate in memory after all."""
import os
import shutil
import tempfile

import pytest

from test_kernel_resources import BUILD, LLVM
from test_kernel_resources_small import _meta

TABLE = 193 * 16
WAVE = (15 * 16 + 15 * 8) * 2
LDS = TABLE + 4 * WAVE  # 5968 bytes
EXPECTED = {"warp_kernel": (2, LDS), "warp_block_kernel": (2, LDS)}


@pytest.fixture(scope="module")
def kernels():
    obj = os.path.join(BUILD, "warp.o")
    if not os.path.exists(os.path.join(LLVM, "clang-offload-bundler")):
        pytest.skip("needs the ROCm LLVM tools")
    assert os.path.exists(obj), "build/warp.o: the library has no warped-motion kernels"
    tmp = tempfile.mkdtemp()
    try:
        return _meta(obj, tmp)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def _named(kernels, name):
    return {n: m for n, m in kernels.items() if str(len(name)) + name + "I" in n}  # the mangled template name


@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_one_instance_per_sample_type_without_scratch_or_spills(kernels, name):
    count, lds = EXPECTED[name]
    mine = _named(kernels, name)
    assert len(mine) == count, sorted(kernels)
    assert any("IhE" in n for n in mine) and any("ItE" in n for n in mine), sorted(mine)
    for n, m in mine.items():
        assert m.get("private_segment_fixed_size", 0) == 0, (n, m)
        assert m.get("vgpr_spill_count", 0) == 0 and m.get("sgpr_spill_count", 0) == 0, (n, m)
        assert m["group_segment_fixed_size"] == lds, (n, m)


VGPRS = {"warp_kernel": 26, "warp_block_kernel": 18}


@pytest.mark.parametrize("name", sorted(VGPRS))
def test_registers_stay_at_the_recorded_figure(kernels, name):
    """One output per lane and two horizontal results: the figures DESIGN.md records, with four registers of margin for a
    compiler update."""
    for n, m in _named(kernels, name).items():
        assert m["vgpr_count"] <= VGPRS[name] + 4, (n, m)


def test_no_other_kernels_in_the_object(kernels):
    assert all(any(_named({n: 0}, k) for k in EXPECTED) for n in kernels), sorted(kernels)
    assert len(kernels) == 4
