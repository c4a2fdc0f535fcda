"""Resources of the inter-intra kernels (CPU test, no GPU), read from the code object in the library's build objects as
test_obmc_pred_resources.py does.  interintra_kernel exists once per sample type and per instance (the predictor; the
four-mode distortion), the two shims' kernels once per sample type, and nothing else is in the object.  A workgroup's LDS is
obmc_pred.hip's: four waves' private slices of pred_plan.h's budget -- the prepared edges reuse the window slice after the
own pass and the weight tables are constant memory, so the kernel adds nothing to it.  The block's inter prediction stays in
registers through the edge step and, in the distortion instance, through the four modes."""
import os
import shutil
import tempfile

import pytest

from test_kernel_resources import BUILD, LLVM
from test_kernel_resources_small import _meta

LDS = 4 * (2112 + 1248) * 2  # 26880 bytes
# kernel -> (instances, LDS bytes, VGPRs as DESIGN.md 3.21 records them)
EXPECTED = {"interintra_kernel": (4, LDS, 95), "blend_a64_mask_kernel": (2, 0, 8), "intra_kernel": (2, 0, 11)}
PREDICT_VGPRS = 60  # the predictor instance alone (Lb0)


@pytest.fixture(scope="module")
def kernels():
    obj = os.path.join(BUILD, "interintra.o")
    if not os.path.exists(os.path.join(LLVM, "clang-offload-bundler")):
        pytest.skip("needs the ROCm LLVM tools")
    assert os.path.exists(obj), "build/interintra.o: the library has no inter-intra kernel"
    tmp = tempfile.mkdtemp()
    try:
        return _meta(obj, tmp)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def _named(kernels, name):
    return {n: m for n, m in kernels.items() if "_N_1" + str(len(name)) + name + "I" in n}


@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_instances_without_scratch_or_spills(kernels, name):
    count, lds, _ = EXPECTED[name]
    mine = _named(kernels, name)
    assert len(mine) == count, sorted(kernels)
    assert any("Ih" in n for n in mine) and any("It" in n for n in mine), sorted(mine)
    for n, m in mine.items():
        assert m.get("private_segment_fixed_size", 0) == 0, (n, m)
        assert m.get("vgpr_spill_count", 0) == 0 and m.get("sgpr_spill_count", 0) == 0, (n, m)
        assert m["group_segment_fixed_size"] == lds, (n, m)


@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_registers_stay_at_the_recorded_figure(kernels, name):
    """The figures DESIGN.md records, with four registers of margin for a compiler update."""
    for n, m in _named(kernels, name).items():
        assert m["vgpr_count"] <= EXPECTED[name][2] + 4, (n, m)
        if name == "interintra_kernel" and "Lb0" in n:
            assert m["vgpr_count"] <= PREDICT_VGPRS + 4, (n, m)


def test_no_other_kernels_in_the_object(kernels):
    assert len(kernels) == 8 and all(any(_named({n: 0}, k) for k in EXPECTED) for n in kernels), sorted(kernels)
