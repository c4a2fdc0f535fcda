"""The three batch predictors (compound, masked compound, warp) share their argument and plane checks (csrc/pred_plan.h):
one table of bad arguments through all three entries on one 64x64 state, the same code from each, pred untouched."""
import ctypes

import numpy as np
import pytest
import torch

import svtgpu

pytestmark = pytest.mark.gpu

W = H = 64
FILL = 5
IDENTITY = [0, 0, 1 << 16, 0, 0, 1 << 16]
OK, INVALID, UNSUPPORTED = 0, -1, -3


def _entries(bd):
    """name -> (call(state, refs, n_refs, block, bit depth, chroma, pred), the valid 8x8 block at (0, 0) with changes)."""
    L = svtgpu.lib()

    def comp(x=0, ref1=1):
        return svtgpu.CompoundBlock.make(x, 0, 8, 8, 0, ref1, (0, 0), (0, 0), 0, 0)

    def masked(x=0, ref1=1):
        return svtgpu.MaskedCompoundBlock.make(x, 0, 8, 8, 0, ref1, (0, 0), (0, 0), 0, 0, 1)

    def warp(x=0, ref1=1):
        return svtgpu.WarpBlock.make(x, 0, 8, 8, 0, IDENTITY, ref1, IDENTITY)
    return {
        "compound": (lambda s, r, n, b, c, p: L.svtgpu_compound_predict_batch(s, r, n, 0, 0, ctypes.byref(b), 1, bd, c, p, None), comp),
        "masked": (lambda s, r, n, b, c, p: L.svtgpu_masked_compound_predict_batch(s, r, n, 0, 0, ctypes.byref(b), 1, bd, c, p, None), masked),
        "warp": (lambda s, r, n, b, c, p: L.svtgpu_warp_predict_batch(s, ctypes.cast(r, ctypes.c_void_p), n, ctypes.byref(b), 1, bd, c, p, None), warp),
    }


@pytest.mark.parametrize("bd", [8, 10])
def test_the_three_entries_refuse_alike(bd):
    ctx = svtgpu.Context(0)
    st = svtgpu.TfState(ctx, W, H)
    dt, bs = (np.uint16, 2) if bd > 8 else (np.uint8, 1)
    tdt = torch.int16 if bd > 8 else torch.uint8
    planes = lambda v: [torch.full((H >> (p > 0), W >> (p > 0)), v, dtype=tdt, device="cuda") for p in range(3)]
    dr, dp = [planes(100), planes(200)], planes(FILL)
    torch.cuda.synchronize()
    strides = [W, W >> 1, W >> 1]
    mk = lambda t, dptr=(0, 0, 0), dstride=(0, 0, 0): svtgpu.TfPlanes.make(
        [(t[p].data_ptr() + dptr[p]) if dptr[p] is not None else None for p in range(3)], [strides[p] + dstride[p] for p in range(3)])
    refs = lambda a=None: (svtgpu.TfPlanes * 27)(*([a or mk(dr[0]), mk(dr[1])] + [mk(dr[0])] * 25))
    pred = mk(dp)
    table = [  # (what, refs, n_refs, block arguments, chroma, pred or None, the code)
        ("27 references", refs(), 27, {}, 1, pred, UNSUPPORTED),
        ("27 references and a null pred", refs(), 27, {}, 1, None, UNSUPPORTED),
        ("a null pred", refs(), 2, {}, 1, None, INVALID),
        ("a null chroma plane with chroma on", refs(mk(dr[0], dptr=(0, None, 0))), 2, {}, 1, pred, INVALID),
        ("a short reference stride", refs(mk(dr[0], dstride=(-1, 0, 0))), 2, {}, 1, pred, INVALID),
        ("a short chroma reference stride", refs(mk(dr[0], dstride=(0, 0, -1))), 2, {}, 1, pred, INVALID),
        ("a misaligned pred", refs(), 2, {}, 1, mk(dp, dptr=(8, 0, 0)), INVALID),
        ("a block one sample past the right edge", refs(), 2, {"x": W - 8 + 1}, 1, pred, INVALID),
        ("a block one step past the right edge", refs(), 2, {"x": W}, 1, pred, INVALID),
        ("ref1 >= n_refs", refs(), 2, {"ref1": 2}, 1, pred, INVALID),
        ("a null chroma plane with chroma off", refs(mk(dr[0], dptr=(0, None, 0))), 2, {}, 0, pred, OK),
    ]
    for name, (call, block) in _entries(bd).items():
        for what, r, n, kw, chroma, p, code in table:
            got = call(st.h, r, n, block(**kw), chroma, ctypes.byref(p) if p is not None else None)
            assert got == code, (name, what, got)
            ctx.synchronize()
            if code != OK:
                assert all((t.cpu().numpy().view(dt) == FILL).all() for t in dp), (name, what)
        assert call(st.h, refs(), 2, block(), 1, ctypes.byref(pred)) == OK, name  # the unchanged arguments are accepted
        ctx.synchronize()
        assert (dp[0].cpu().numpy().view(dt)[:8, :8] != FILL).all(), name
        for t in dp:
            t.fill_(FILL)
        torch.cuda.synchronize()
    st.close()
