"""Resources of the small instances of the resident searches (CPU test, no GPU), read from the code object in the
library's build objects as test_kernel_resources.py does.  wiener_res_small_kernel (256 lanes, a window of at most
38 KB) exists to hold four workgroups of 128 x 128 chroma units on a CU that the big instance reserves whole: per
workgroup one wave per SIMD, so at most 128 VGPRs, and a quarter of the CU's LDS, with no scratch.  sgr_res_small_kernel exists to hold three workgroups
of 128 x 128 chroma items on a CU where the big instance holds two: that needs, per 512-lane workgroup, at most 80
VGPRs (6 waves per SIMD of a 512-register file, allocated in eights) and a third of the CU's 160 KB of LDS -- and, as
for every resident descent, no scratch at all.  (Four per CU, 64 VGPRs, was the target: the compiler spilled 54 to 79
registers of the load phase there.)"""
import os
import shutil
import tempfile

import pytest

from test_kernel_resources import BUILD, LLVM, _kernels

WGS_PER_CU = 3          # what the implementation settled on (SVTGPU_SRS_WGS)
LANES = 512             # SR_NT
DYN_LDS = 10 * 448 * 8  # SRS_KMAX chunks x 448 pixel lanes x 8 bytes of (x - src): the launch's dynamic LDS
CU_LDS = 160 * 1024
SIMD_VGPRS = 512


def _meta(obj, tmp):
    """_kernels() plus the static LDS size of every kernel."""
    import re
    import subprocess
    ks = _kernels(obj, tmp)
    notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", os.path.join(tmp, "k.co")], check=True,
                           capture_output=True, text=True).stdout
    lds = None  # a kernel's entry lists its keys in alphabetical order: the LDS size comes before the name
    for line in notes.splitlines():
        m = re.match(r"\s+\.group_segment_fixed_size:\s+(\d+)", line)
        if m:
            lds = int(m.group(1))
        m = re.match(r"\s+\.name:\s+(\S+)", line)
        if m and m.group(1) in ks and lds is not None:
            ks[m.group(1)]["group_segment_fixed_size"] = lds
            lds = None
    return ks


@pytest.fixture(scope="module")
def small_kernels():
    if not os.path.isdir(BUILD) or not os.path.exists(os.path.join(LLVM, "clang-offload-bundler")):
        pytest.skip("needs the built objects and the ROCm LLVM tools")
    tmp = tempfile.mkdtemp()
    try:
        ks = _meta(os.path.join(BUILD, "lr_search.o"), tmp)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return {n: m for n, m in ks.items() if "sgr_res_small_kernel" in n}


@pytest.fixture(scope="module")
def wiener_small_kernels():
    if not os.path.isdir(BUILD) or not os.path.exists(os.path.join(LLVM, "clang-offload-bundler")):
        pytest.skip("needs the built objects and the ROCm LLVM tools")
    tmp = tempfile.mkdtemp()
    try:
        ks = _meta(os.path.join(BUILD, "lr_search.o"), tmp)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return {n: m for n, m in ks.items() if "wiener_res_small_kernel" in n}


WR_WGS_PER_CU, WR_LANES, WR_DYN_LDS = 4, 256, 38 * 1024  # WRS_NT, WRS_LDS_CAP: the largest window of a small unit


def test_wiener_small_instance(wiener_small_kernels):
    ks = wiener_small_kernels
    assert len(ks) == 2 and any("IhL" in n for n in ks) and any("ItL" in n for n in ks), sorted(ks)
    assert not any("wiener_res_kernel" in n for n in ks)
    waves_per_simd = WR_WGS_PER_CU * (WR_LANES // 64) // 4
    for n, m in ks.items():
        assert m.get("private_segment_fixed_size", 0) == 0 and m.get("vgpr_spill_count", 0) == 0, (n, m)
        assert (m["vgpr_count"] + 7) // 8 * 8 * waves_per_simd <= SIMD_VGPRS, (n, m)
        assert (m["group_segment_fixed_size"] + WR_DYN_LDS) * WR_WGS_PER_CU <= CU_LDS, (n, m)


def test_small_instance_exists_for_both_sample_types(small_kernels):
    # one instantiation per sample type: uint8_t (Ih) and uint16_t (It)
    assert len(small_kernels) == 2, sorted(small_kernels)
    assert any("IhE" in n for n in small_kernels) and any("ItE" in n for n in small_kernels), sorted(small_kernels)
    # the old names still match exactly the old kernels (test_kernel_resources.py counts them)
    assert not any("sgr_res_kernel" in n or "wiener_res_kernel" in n for n in small_kernels)


def test_small_instance_keeps_to_registers(small_kernels):
    assert small_kernels
    for n, m in small_kernels.items():
        assert m.get("private_segment_fixed_size", 0) == 0, (n, m)
        assert m.get("vgpr_spill_count", 0) == 0 and m.get("sgpr_spill_count", 0) == 0, (n, m)


def test_small_instance_fits_three_workgroups_per_cu(small_kernels):
    assert small_kernels
    waves_per_simd = WGS_PER_CU * (LANES // 64) // 4
    for n, m in small_kernels.items():
        assert (m["vgpr_count"] + 7) // 8 * 8 * waves_per_simd <= SIMD_VGPRS, (n, m)
        assert (m["group_segment_fixed_size"] + DYN_LDS) * WGS_PER_CU <= CU_LDS, (n, m)
