"""Resources of the OBMC prediction kernel (CPU test, no GPU), read from the code object in the library's build objects as
test_warp_resources.py does.  obmc_pred_kernel and the blend shims' kernel exist once per sample type, the weighted-source kernel once (8 bits), and
nothing else is in the object.  A
workgroup's LDS is four waves' private slices of pred_plan.h's budget (window and intermediate, 16 bits each); the block's
own prediction stays in registers through every neighbour pass, so scratch would be that value in memory after all."""
import os
import shutil
import tempfile

import pytest

from test_kernel_resources import BUILD, LLVM
from test_kernel_resources_small import _meta

LDS = 4 * (2112 + 1248) * 2  # 26880 bytes
# kernel -> (instances, LDS bytes, VGPRs as DESIGN.md 3.20 records them)
EXPECTED = {"obmc_pred_kernel": (2, LDS, 147), "obmc_wsrc_kernel": (1, LDS, 159), "blend_mask_kernel": (2, 0, 6)}


@pytest.fixture(scope="module")
def kernels():
    obj = os.path.join(BUILD, "obmc_pred.o")
    if not os.path.exists(os.path.join(LLVM, "clang-offload-bundler")):
        pytest.skip("needs the ROCm LLVM tools")
    assert os.path.exists(obj), "build/obmc_pred.o: the library has no OBMC prediction kernel"
    tmp = tempfile.mkdtemp()
    try:
        return _meta(obj, tmp)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def _named(kernels, name):
    return {n: m for n, m in kernels.items() if str(len(name)) + name in n}


@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_instances_without_scratch_or_spills(kernels, name):
    count, lds, _ = EXPECTED[name]
    mine = _named(kernels, name)
    assert len(mine) == count, sorted(kernels)
    if count == 2:
        assert any("IhE" in n for n in mine) and any("ItE" in n for n in mine), sorted(mine)
    for n, m in mine.items():
        assert m.get("private_segment_fixed_size", 0) == 0, (n, m)
        assert m.get("vgpr_spill_count", 0) == 0 and m.get("sgpr_spill_count", 0) == 0, (n, m)
        assert m["group_segment_fixed_size"] == lds, (n, m)


@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_registers_stay_at_the_recorded_figure(kernels, name):
    """The figures DESIGN.md records, with four registers of margin for a compiler update."""
    for n, m in _named(kernels, name).items():
        assert m["vgpr_count"] <= EXPECTED[name][2] + 4, (n, m)


def test_no_other_kernels_in_the_object(kernels):
    assert len(kernels) == 5 and all(any(_named({n: 0}, k) for k in EXPECTED) for n in kernels), sorted(kernels)
