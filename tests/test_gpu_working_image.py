"""The working image of the extract stage on the device - BGR to grey, cv::resize(INTER_AREA) to a long side of 1600,
(float)u8 * (1 / 255f): csrc/akaze.hip, working_image_enqueue - through the seam ochip_debug_working_image, which runs the
function akaze_run runs and nothing after it, and reports the kernels it launched.  Per case of
tests/working_image_fixtures.py: the reported route is the one the fixtures' restated dispatch expects, the floats are
(float)u8 * (1 / 255f) of an 8-bit image to the bit, that image is bit-equal to the restatement (oracle.gray_resize) and
passes the comparison rule against the float64 model (tests/test_working_image_oracle.py holds the restatement against the
same model without a device), and every route that can take one source gives the same bits: host and device input, a
device buffer off 4-byte alignment by 1, 2 and 3 bytes, a member of a batch and the image alone.  AKAZE never runs."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import working_image_fixtures as wf
from opencalibration_amd import capi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


@contextlib.contextmanager
def device_bytes(ctx, data):
    """The address of a copy of `data` (uint8) in device memory, 256-byte aligned: one image slot of the context
    (include/ochip.h: ochip_image_slots_*), handed back on exit."""
    L = ctx.L
    L.ochip_image_slots_create.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint32, C.POINTER(C.c_void_p)]
    L.ochip_image_slots_upload.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64]
    L.ochip_image_slots_mark.argtypes = [C.c_void_p, C.c_uint32]
    L.ochip_image_slots_wait.argtypes = [C.c_void_p, C.c_uint32, C.c_int]
    L.ochip_image_slots_address.argtypes = [C.c_void_p, C.c_uint32]
    L.ochip_image_slots_address.restype = C.c_uint64
    L.ochip_image_slots_destroy.argtypes = [C.c_void_p]
    L.ochip_image_slots_destroy.restype = None
    slots = C.c_void_p()
    ctx._check(L.ochip_image_slots_create(ctx.h, 1, data.size, 1, C.byref(slots)), "ochip_image_slots_create")
    try:
        ctx._check(L.ochip_image_slots_upload(slots, 0, data.ctypes.data, data.size), "ochip_image_slots_upload")
        ctx._check(L.ochip_image_slots_mark(slots, 0), "ochip_image_slots_mark")
        ctx._check(L.ochip_image_slots_wait(slots, 0, 1), "ochip_image_slots_wait")
        address = int(L.ochip_image_slots_address(slots, 0))
        assert address and address % 4 == 0
        yield address
    finally:
        L.ochip_image_slots_destroy(slots)


@pytest.fixture(scope="module")
def run(ctx):
    """run(names, offset): the seam on the images of `names` as one batch - from host memory (offset None) or from a device
    buffer `offset` bytes past a 4-byte aligned address.  Every distinct call runs once."""
    done = {}

    def go(names, offset=None):
        key = (tuple(names), offset)
        if key not in done:
            batch = np.stack([wf.built(n)[0] for n in names])
            if offset is None:
                out = ctx.working_image(batch)
            else:
                shifted = np.zeros(batch.size + 8, np.uint8)
                shifted[offset:offset + batch.size] = batch.reshape(-1)
                with device_bytes(ctx, shifted) as address:
                    out = ctx.working_image(None, device_ptr=address + offset, shape=batch.shape[:3])
            out[0].setflags(write=False)
            done[key] = out
        return done[key]

    go.done = done
    return go


@pytest.mark.parametrize("case", wf.CASES, ids=repr)
def test_working_image(case, run, oracle):
    img, model = wf.built(case.name)
    floats, wh, resize, grey = run([case.name])
    assert wh == (model.W, model.H) and floats.shape == (1, model.H, model.W)
    assert (resize, grey) == wf.routes(model, aligned=True) == (case.resize, case.grey), (wf.RESIZE_NAMES[resize], wf.GREY_NAMES[grey])
    u8 = wf.u8_of(floats[0])
    assert np.array_equal(u8, oracle.gray_resize(img, model.W, model.H))
    f = wf.check(u8, model)
    print(f"WORKING_IMAGE_FIGURES device {case.name}: {wf.RESIZE_NAMES[resize]} / {wf.GREY_NAMES[grey]}, band {100 * f['band_share']:.3f} %, "
          f"worst outside {f['worst_outside']:.6f}, wrong outside {f['wrong_outside']}, worst levels {f['worst_levels']}")
    assert wf.passed(f), f


@pytest.mark.parametrize("case,offset", [(c, o) for c in wf.CASES for o in c.offsets], ids=repr)
def test_a_source_off_alignment_gives_the_same_bits(case, offset, run):
    """A device pointer that is no multiple of 4 cannot be read by dwords: the grey image is made byte by byte and the resize,
    where it stages, stages from it."""
    model = wf.built(case.name)[1]
    want = run([case.name])
    floats, wh, resize, grey = run([case.name], offset)
    assert (resize, grey) == wf.routes(model, aligned=False) and grey == wf.GREY_BYTEWISE
    assert resize == {wf.RESIZE_FUSED4: wf.RESIZE_STAGED_GREY, wf.RESIZE_FUSED8: wf.RESIZE_STAGED_GREY}.get(case.resize, case.resize)
    assert wh == want[1] and np.array_equal(floats.view(np.uint32), want[0].view(np.uint32))


def test_host_and_device_input_agree(run):
    name = wf.CASES[0].name
    want = run([name])
    got = run([name], 0)
    assert got[1:] == want[1:] and np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32))


@pytest.mark.parametrize("offset", [None, 0, 1], ids=["host", "device", "device+1"])
def test_a_batch_member_is_the_image_alone(offset, run):
    """Three different images of the headline shape in one call: the kernels' blockIdx.z offsets into source, grey image
    and destination."""
    names = list(wf.BATCH)
    floats, wh, resize, grey = run(names, offset)
    model = wf.built(names[0])[1]
    assert (resize, grey) == wf.routes(model, aligned=offset != 1, n_images=3)
    assert resize == (wf.RESIZE_STAGED_GREY if offset == 1 else wf.RESIZE_FUSED4)
    for k, name in enumerate(names):
        alone = run([name])
        assert wh == alone[1] and np.array_equal(floats[k].view(np.uint32), alone[0][0].view(np.uint32)), name


def test_every_route_is_reported(run):
    for case in wf.CASES:
        run([case.name])
        for offset in case.offsets:
            run([case.name], offset)
    seen_resize = {out[2] for out in run.done.values()}
    seen_grey = {out[3] for out in run.done.values()}
    assert seen_resize == {wf.RESIZE_NONE, wf.RESIZE_FUSED4, wf.RESIZE_FUSED8, wf.RESIZE_STAGED_GREY, wf.RESIZE_PER_TAP}
    assert seen_grey == {wf.GREY_FUSED, wf.GREY_GRAY4, wf.GREY_GRAY4_TAIL, wf.GREY_BYTEWISE}


def test_the_seam_refuses_bad_arguments(ctx):
    with pytest.raises(capi.OchipError):
        ctx.working_image(np.zeros((1, 0, 4, 3), np.uint8))
    out, wh, resize, grey = ctx.working_image(np.zeros((0, 8, 8, 3), np.uint8))
    assert out.shape == (0, 8, 8) and wh == (8, 8)
