"""The inter-intra RTCD install (include/svtgpu_rtcd.h, SVTGPU_RTCD_WITH_INTERINTRA) against the reference's own
declarations, as tests/test_obmc_blend_rtcd.py checks the OBMC blends: compile-and-link on the CPU, pointer comparisons
only."""
import os
import subprocess
import tempfile

import pytest

import svtgpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
S = os.path.join(REF, "Source")
REF_OBJ = os.path.join(ROOT, "oracle", "_ref", "obj")
LIB_DIR = os.path.dirname(svtgpu.LIB_PATH)
INC = ["-I" + os.path.join(S, d) for d in
       ("API", "Lib/Common/Codec", "Lib/Common/C_DEFAULT", "Lib/Encoder/Codec", "Lib/Encoder/C_DEFAULT",
        "Lib/Encoder/Globals", "Lib/Common/ASM_AVX2", "Lib/Encoder/ASM_AVX2", "Lib/Common/ASM_SSE2",
        "Lib/Common/ASM_SSE4_1")] + \
      ["-I" + os.path.join(REF, "third_party/aom/inc"), "-I" + os.path.join(REF, "third_party/cpuinfo/include"),
       "-I" + REF, "-I" + os.path.join(ROOT, "include")]
STRICT = ["-DARCH_X86_64=1", "-Werror=incompatible-pointer-types", "-Werror=discarded-qualifiers"]


@pytest.mark.skipif(not (os.path.isdir(S) and os.path.exists(os.path.join(REF_OBJ, "Lib/Encoder/Codec/aom_dsp_rtcd.o"))),
                    reason="oracle/_ref/obj not built (needs /root/reference)")
def test_interintra_install_sets_every_pointer():
    """The adapters and svtgpu_install_interintra_rtcd() compile as C without a cast under
    -Werror=incompatible-pointer-types, and the install leaves the two blends and the 140 per-size predictors (seven kinds,
    ten plane sizes, two depths) on the library's side."""
    objs = [os.path.join(REF_OBJ, p) for p in ("Lib/Encoder/Codec/aom_dsp_rtcd.o", "Lib/Common/Codec/common_dsp_rtcd.o",
                                               "Lib/Common/Codec/EbUtility.o")]
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "interintra_install")
        r = subprocess.run(["gcc", "-O1", "-fPIC", "-ffunction-sections", "-fdata-sections"] + STRICT + INC +
                           [os.path.join(ROOT, "tests", "interintra_install.c")] + objs +
                           ["-o", exe, "-Wl,--gc-sections", "-L" + LIB_DIR, "-lsvtgpu", "-Wl,-rpath," + LIB_DIR, "-ldl",
                            "-lm", "-lpthread"], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
        res = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, res.stderr[-2000:]
    assert res.stdout.split() == ["before", "0/142", "after", "142/142"], res.stdout
