"""Super-resolution without a GPU: the numpy restatement of tests/superres_cases.py against every upscale record of the
reference's fixture (the checker the GPU tests rely on), and the library's two host-only helpers against every
recorded value."""
import ctypes

import numpy as np
import pytest

import superres_cases as sc
import svtgpu

UP = list(sc.up_cases())


def test_fixture_covers_the_cases():
    assert {(c["denom"], c["bd"], c["sub_x"]) for c in UP if c["upscaled_width"] == 88 and c["rows"] in (8, 16)} >= \
        {(d, bd, sx) for d in range(9, 17) for bd in (8, 10) for sx in (0, 1)}
    assert any(c["out_w"] == 42 for c in UP) and any(c["in_w"] == 313 and c["coded"] == 320 for c in UP)
    assert any(c["ntile"] == 2 and c["in_w"] == 139 and c["coded"] == 144 for c in UP)
    assert any(c["out_w"] == 3840 and c["in_w"] == 1920 and c["bd"] == 10 for c in UP)
    for bd in (8, 10):  # the extreme content: sums beyond both clips, and flat max stays max
        maxv = (1 << bd) - 1
        ext = [c for c in UP if c["bd"] == bd and c["rows"] >= 6 and (c["src"][3] == maxv).all()]
        assert len(ext) >= 3 and all((c["out"][3] == maxv).all() for c in ext)
        for c in ext:
            raw = sc.upscale_plane(c["src"], c["in_w"], c["out_w"], bd, clip=False)
            assert raw.min() < 0 and raw.max() > maxv, c["name"]


@pytest.mark.parametrize("i", range(len(UP)))
def test_restatement_matches_upscale_records(i):
    c = UP[i]
    assert sc.scaled_size(c["upscaled_width"], c["denom"]) == c["frame_width"]
    got = sc.upscale_plane(c["src"], c["in_w"], c["out_w"], c["bd"])
    np.testing.assert_array_equal(got, c["out"], err_msg=c["name"])


def test_scaled_size_matches_reference():
    g = sc.fixture()
    L = svtgpu.lib()
    for i, dim in enumerate(int(v) for v in g["scaled_dims"]):
        for j, denom in enumerate(sc.DENOMS):
            want = int(g["scaled"][i][j])
            assert L.svtgpu_superres_scaled_size(dim, denom) == want == sc.scaled_size(dim, denom), (dim, denom)
            assert svtgpu.superres_scaled_size(dim, denom) == want
    assert [int(v) for v in g["scaled"][:, 0]] == [int(v) for v in g["scaled_dims"]]  # denominator 8: unchanged


def test_geometry_matches_reference():
    g = sc.fixture()
    L = svtgpu.lib()
    assert len(g["geom"]) == len(UP)
    for in_w, out_w, step, x0 in (tuple(int(v) for v in row) for row in g["geom"]):
        a, b = ctypes.c_int32(-1), ctypes.c_int32(-1)
        assert L.svtgpu_superres_geometry(in_w, out_w, ctypes.byref(a), ctypes.byref(b)) == 0
        assert (a.value, b.value) == (step, x0) == sc.geometry(in_w, out_w) == svtgpu.superres_geometry(in_w, out_w)
    a = ctypes.c_int32(0)
    assert L.svtgpu_superres_geometry(0, 8, ctypes.byref(a), ctypes.byref(a)) == -1
    assert L.svtgpu_superres_geometry(8, 16, None, ctypes.byref(a)) == -1


def test_abi_version_and_symbols():
    assert svtgpu.lib().svtgpu_abi_version() >= 10
    names = ["svtgpu_superres_scaled_size", "svtgpu_superres_geometry", "svtgpu_superres_upscale_plane",
             "svtgpu_superres_upscale_frame"]
    assert all(n in svtgpu._SIGS and n in svtgpu.declared_symbols() for n in names)
