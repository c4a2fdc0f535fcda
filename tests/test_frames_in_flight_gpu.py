"""Frames in flight and stage states reused from frame to frame: bench.py's shape (one DlfState / CdefState / LrState
per slot that persist from step to step, one stream and one thread per slot, the asynchronous forms with the host
running ahead of the device), every frame bit-exact against the reference's goldens through pipeline_run.check().
The frames are the groups of pipeline_cases.GROUPS -- cases of one size whose consecutive members differ in every
decision and every output plane (tests/test_frames_in_flight.py) -- so a result kept from the frame before fails.

The one-line library changes each test catches and the suite before it did not, reasoned from the code, NOT RUN (no
mutated kernel was built):
* test_sequence_on_one_state: cdef_pick_common without its hipMemsetAsync of d_fb_strength for a reference-strength
  frame (cdef_api.hip: after a searched frame the apply then indexes the one strength pair with the frame before's
  per-block indices; the 256x192 pair and the 8-bit group -- a fresh state's indices are zero, so no test saw it);
  svtgpu_cdef_pick_impl without the `pick_xch_end != end` clear of the pick's exchange words when the strength
  count changes (cdef_pick.hip; 48 -> 20 -> 9 strengths in the 320x200 group; it matters only when the asynchronous
  pick's fallback runs, i.e. a chain is unsettled at the check); svtgpu_cdef_pick_read taking the strength map of
  the pick before (apick_map saved before, not after, the launch of another level's pick).
* test_run_ahead: svtgpu_dlf_pick_async copying the start plan into plans[1] instead of plans[0], or its trial
  launches all reading plans[0] (the double buffer of dlf.hip: a late workgroup of a round then reads the plan the
  round's step has rewritten -- with three searches queued back to back the next frame's rounds follow at once);
  svtgpu_dlf_set_mode_info without its wait on mi_free (frame 2's grid overwrites the staging buffer frame 1's copy
  has not read yet: the host form), or the LR search without its wait on pin_free (frame 2's plan overwrites the
  page-locked buffer frame 1's upload has not read yet; the 320x200 group's LR levels give every frame another
  plan); the CDEF strength map or the level search's start parameters moved from kernel
  arguments into a per-state host buffer that a queued kernel reads after the next frame's call has rewritten it.
* test_four_slots: a buffer shared between states that should be per state (a static scratch pointer in lr_search.hip
  or dlf.hip), a kernel launched on the context's stream instead of the caller's (the slot's collect then reads
  planes the other stream has not written), the persistent pick fallback's exchange words shared between states.
* test_ready_flags: removing `s->dev_ready = 0` from svtgpu_dlf_pick or `s->apick_ready = 0` from cdef_pick_common:
  the NULL-parameter filter / apply then silently uses frame A's device result for frame B.  On the parent commit
  this test fails (neither flag was ever cleared: both calls return SVTGPU_OK).
"""
import threading

import pytest

import pipeline_cases as pc
import pipeline_run as prun

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

FORMS = {"async": lambda i: True, "sync": lambda i: False, "alternate": lambda i: i % 2 == 0}
STARTS = [(g, s) for g, names in pc.GROUPS.items() for s in range(len(names))]


@pytest.fixture(scope="module")
def ctx():
    import svtgpu
    return svtgpu.Context(0)


@pytest.fixture(scope="module")
def streams(ctx):
    """Four library streams, the frames-in-flight count of the benchmark (one hardware queue each)."""
    s = [ctx.stream_create(0) for _ in range(4)]
    yield s
    for p in s:
        ctx.stream_destroy(p)


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("group", list(pc.GROUPS))
def test_sequence_on_one_state(ctx, streams, group, form):
    """A, B, C, A, B (a pair: A, B, A, B, A) on one slot, every frame collected before the next: each frame's levels,
    CDEF tables / parameters / strengths, LR frame types / units and planes equal its golden -- in the asynchronous
    forms, the synchronous forms, and alternating per frame (async, sync, async, ...)."""
    names = pc.sequence(group)
    slot = prun.FrameSlot.for_case(ctx, names[0], streams[0])
    for i, name in enumerate(names):
        out = slot.collect(slot.enqueue(name, FORMS[form](i)), last=True)
        assert not out["planes_only"]
        prun.check(name, out, "%s frame %d of %s" % (form, i, group))
    slot.close()


@pytest.mark.parametrize("mi", ["device", "host"])
@pytest.mark.parametrize("group,start", STARTS)
def test_run_ahead(ctx, streams, group, start, mi):
    """Three frames of the asynchronous form enqueued on one slot behind a 40 ms stall of its stream with no collect
    between them, after one frame that was collected (so no first-call allocation is left).  Every frame's planes
    and the last frame's decisions equal the goldens; every case of a group is the last frame once.
    What waits on the host by design (FrameSlot's header), found with this test's first run: the LR search of frame
    2 waits until frame 1 has reached its LR stage (pin_free), so frame 1 whole and frame 2's DLF and CDEF stages --
    uploads, mode info, block mask, controls, the level search's plans, the pick's strength map -- are written
    before a kernel of frame 1 has run, and frame 3 beside frame 2's kernels.  With the host grid
    svtgpu_dlf_set_mode_info of frame 2 already waits for frame 1's copy (mi_free); with the device grid the
    explicit-level filter of an SB-based DLF case waits for the grid's verdict.  Asserted: with the device grid and a
    device level search, frame 1 reaches its LR stage with the stall still holding the stream, so every call up to
    there queues.  Not asserted: that frame 2 gets as far (on the first runs it did from two of the 320x200 group's
    three starts; with mini10 as frame 2 the stall had ended by then, the cause not established)."""
    import torch

    class Probe:  # FrameSlot.enqueue's at_lr hook: is the stall still holding the stream?
        held = None

        def set(self):
            self.held = not behind.query()
    names = pc.sequence(group, start, 4)
    slot = prun.FrameSlot.for_case(ctx, names[0], streams[0], mi_device=mi == "device")
    for n in names:
        prun.case_inputs(n, mi == "device")
    prun.check(names[0], slot.collect(slot.enqueue(names[0], True), last=True), "run-ahead warm-up")
    ext = torch.cuda.ExternalStream(streams[0])
    ctx.debug_stall(40, streams[0])
    behind = torch.cuda.Event()
    behind.record(ext)
    probes = [Probe() for _ in names[1:]]
    steps = [slot.enqueue(n, True, p) for n, p in zip(names[1:], probes)]
    outs = [slot.collect(hd, last=hd is steps[-1]) for hd in steps]
    slot.close()
    for i, (n, out) in enumerate(zip(names[1:], outs)):
        assert out["planes_only"] == (i < 2)
        prun.check(n, out, "run-ahead frame %d of %s from %d (%s grid)" % (i, group, start, mi))
    if mi == "device" and not prun.dlf_ctrls(pc.CASES[names[1]]["dlf_level"])["sb_based"]:
        assert probes[0].held, "a call of the asynchronous form before frame 1's LR stage waited on the host"


def _run_slots(ctx, streams, plans, async_, steps=6, run_ahead=2):
    """bench.py's run(): one thread per slot, slot k starting when slot k - 1 reaches its LR stage, each thread at
    most `run_ahead` steps ahead of its stream.  The first error stops every slot before its next library call and is
    re-raised here; after an error nothing more is started on the device (no collect, no close)."""
    slots = [prun.FrameSlot.for_case(ctx, names[0], streams[k]) for k, names in enumerate(plans)]
    for names in plans:
        for n in set(names):
            prun.case_inputs(n)
    at_lr = [threading.Event() for _ in slots]
    stop, errors, done = threading.Event(), [], []

    def run(k):
        try:
            if k > 0:
                at_lr[k - 1].wait(60)  # bounded: a failed slot must not hang the next
            pending = []
            for i in range(steps + run_ahead):
                if i < steps:
                    if stop.is_set():
                        return
                    pending.append((i, slots[k].enqueue(plans[k][i], async_, at_lr[k])))
                if len(pending) > run_ahead or i >= steps:
                    if stop.is_set():
                        return
                    j, hd = pending.pop(0)
                    out = slots[k].collect(hd, last=j == steps - 1)
                    assert out["planes_only"] == (async_ and j < steps - 1)
                    prun.check(plans[k][j], out, "slot %d step %d" % (k, j))
                    done.append((k, j))
        except BaseException as e:  # re-raised on the main thread
            errors.append(e)
            stop.set()
            at_lr[k].set()

    threads = [threading.Thread(target=run, args=(k,), daemon=True) for k in range(len(slots))]
    for t in threads:
        t.start()
    for t in threads:
        t.join(120)
    if errors:
        raise errors[0]
    assert not any(t.is_alive() for t in threads), "a slot's thread did not finish within its bound"
    assert sorted(done) == [(k, j) for k in range(len(slots)) for j in range(steps)]
    for s in slots:
        s.close()


@pytest.mark.parametrize("form", ["async", "sync"])
def test_four_slots(ctx, streams, form):
    """Four slots at once, one thread and one library stream each: the 320x200 group, the 256x192 pair, the 8-bit
    200x136 group, and sb128_10 repeated (whose svtgpu_cdef_set_fb_bsize waits for its stream every frame, by
    design).  Six steps a slot, two steps of run-ahead, staggered starts: every step's planes and every slot's last
    decisions equal the goldens, in the asynchronous and in the synchronous forms."""
    plans = [pc.sequence("320x200_10", 0, 6), pc.sequence("256x192_10", 0, 6), pc.sequence("200x136_8", 0, 6),
             ["sb128_10"] * 6]
    _run_slots(ctx, streams, plans, form == "async")


def test_ready_flags(ctx, streams):
    """Frame A with the asynchronous picks, then frame B with the synchronous svtgpu_dlf_pick and svtgpu_cdef_pick on
    the same states: B applied with its explicit parameters equals B's golden, and the NULL-parameter forms, which
    refer to the last asynchronous pick with nothing in between, now refuse (SvtGpuError) instead of filtering B with
    A's levels and strengths; so do the read-backs of the asynchronous results."""
    import svtgpu
    a, b = "mini10", "seq10_b"
    assert not prun.dlf_ctrls(pc.CASES[a]["dlf_level"])["sb_based"] and not prun.dlf_ctrls(pc.CASES[b]["dlf_level"])["sb_based"]
    slot = prun.FrameSlot.for_case(ctx, a, streams[0])
    prun.check(a, slot.collect(slot.enqueue(a, True), last=True), "ready flags, frame A (async)")
    hd = slot.enqueue(b, False)
    prun.check(b, slot.collect(hd, last=True), "ready flags, frame B (sync)")
    D, C, O = hd["outs"]
    with pytest.raises(svtgpu.SvtGpuError):
        slot.st.apply(D, C, None, streams[0])
    with pytest.raises(svtgpu.SvtGpuError):
        slot.dl.filter_to(slot.R, D, None, stream=streams[0])
    with pytest.raises(svtgpu.SvtGpuError):
        slot.dl.filter(D, None, stream=streams[0])
    with pytest.raises(svtgpu.SvtGpuError):
        slot.st.read_params(streams[0])
    with pytest.raises(svtgpu.SvtGpuError):
        slot.dl.read_levels(streams[0])
    # the next asynchronous picks arm them again
    prun.check(a, slot.collect(slot.enqueue(a, True), last=True), "ready flags, frame A again (async)")
    slot.close()
