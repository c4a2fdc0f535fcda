"""Resources of the masked compound kernels (CPU test, no GPU), read from the code object in the library's build objects
as test_compound_resources.py does.  masked_compound_kernel (the batch: 256 lanes, four waves with compound_kernel's
private LDS slice each) and blend_d16_kernel (the two blend shims) exist for both sample types, diffwtd_mask_kernel (the
mask shim, which sees only CONV_BUF_TYPE values) once; nothing else is in the object.  The batch kernel holds both
references' CONV_BUF_TYPE values of a lane in registers until the blend, so scratch there would be the intermediate in
memory after all."""
import os
import shutil
import tempfile

import pytest

from test_compound_resources import WAVE_LDS
from test_kernel_resources import BUILD, LLVM
from test_kernel_resources_small import _meta

EXPECTED = {"masked_compound_kernel": (2, 4 * WAVE_LDS), "blend_d16_kernel": (2, 0), "diffwtd_mask_kernel": (1, 0)}


@pytest.fixture(scope="module")
def kernels():
    obj = os.path.join(BUILD, "masked_compound.o")
    if not os.path.exists(obj) or not os.path.exists(os.path.join(LLVM, "clang-offload-bundler")):
        pytest.skip("needs the built objects and the ROCm LLVM tools")
    tmp = tempfile.mkdtemp()
    try:
        return _meta(obj, tmp)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_one_instance_per_sample_type_without_scratch_or_spills(kernels, name):
    count, lds = EXPECTED[name]
    mine = {n: m for n, m in kernels.items() if name in n}
    assert len(mine) == count, sorted(kernels)
    if count == 2:
        assert any("IhE" in n for n in mine) and any("ItE" in n for n in mine), sorted(mine)
    for n, m in mine.items():
        assert m.get("private_segment_fixed_size", 0) == 0, (n, m)
        assert m.get("vgpr_spill_count", 0) == 0 and m.get("sgpr_spill_count", 0) == 0, (n, m)
        assert m["group_segment_fixed_size"] == lds, (n, m)


def test_the_batch_kernel_needs_no_more_registers_than_the_compound_kernel(kernels):
    """compound_kernel takes 163 VGPRs (three waves per SIMD); the masked kernel must not fall to two."""
    for n, m in kernels.items():
        if "masked_compound_kernel" in n:
            assert m["vgpr_count"] <= 168, (n, m)


def test_no_other_kernels_in_the_object(kernels):
    assert all(any(k in n for k in EXPECTED) for n in kernels), sorted(kernels)
    assert len(kernels) == 5
