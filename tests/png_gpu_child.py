"""The scenarios of test_gpu_png.py, run in a child process that brings torch up before libochip.so (as geotiff_gpu_child.py
does) and holds one capi.Context(0).  `python png_gpu_child.py <tests dir> <repo dir>` runs every scenario and prints one
JSON line {scenario: "ok" or the failure's traceback}.  A scenario that ends in a device error ends the run: the ones after it
are reported as not run.  The yardstick is the CPU route of the same library (ctx None), which test_png_host.py holds against
Pillow and zlib.  No scenario feeds a kernel a broken input: the refusals go through the entry points."""
import base64
import io
import json
import sys
import traceback

import numpy as np
import torch

torch.cuda.init()
if __name__ == "__main__":
    sys.path[:0] = sys.argv[1:3]

import png_fixtures as F  # noqa: E402
from layers_fixtures import four_camera_scene  # noqa: E402
from tile_progress_fixtures import difference, mosaic_plan  # noqa: E402
from opencalibration_amd import capi, host  # noqa: E402

MOSAIC = (0.05, 160, 1)  # gsd, tile_size, tile_rows: the smallest scene of the mosaic GPU tests, 210 x 180
COPIES = 1000


def to_device(a):
    t = torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    torch.cuda.synchronize()  # the kernels run on the context's own stream
    return t


def same(got, want, what):
    assert len(got) == len(want), f"{what}: {len(got)} results against {len(want)}"
    for k, (g, w) in enumerate(zip(got, want)):
        if g != w:
            at = next((i for i, (a, b) in enumerate(zip(g, w)) if a != b), min(len(g), len(w)))
            raise AssertionError(f"{what}, image {k}: {len(g)} bytes against {len(w)}, first difference at byte {at}")


def scenario_one_by_one(ctx):
    cpu, dev = host.PngEncoder(), host.PngEncoder(ctx)
    for name in F.ALL:
        a = F.image(name)
        d = to_device(a)
        for bgr in (False, True):
            want = cpu.encode([a], bgr=bgr)
            same(dev.encode([a], bgr=bgr), want, f"{name} bgr={bgr}: numpy through the device")
            same(dev.encode([d], bgr=bgr), want, f"{name} bgr={bgr}: a CUDA tensor")
        want = cpu.encode([a], base64=True)
        same(dev.encode([d], base64=True), want, f"{name}: base64")
        assert want[0] == base64.b64encode(cpu.encode([a])[0]).decode()
    same([host.encode_png(to_device(F.image("thumb_noisy")), ctx=ctx)], [host.encode_png(F.image("thumb_noisy"))], "encode_png")
    f = io.BytesIO()
    host.save_png(f, to_device(F.image("rgba_photo")), ctx=ctx, bgr=True)
    same([f.getvalue()], [host.encode_png(F.image("rgba_photo"), bgr=True)], "save_png")
    cpu.close(), dev.close()


def scenario_mixed_batch(ctx):
    """every fixture and 1 000 thumbnails in one call: small and large images, one, three and four channels, deflated and stored"""
    batch = [F.image(k) for k in F.ALL[:6]] + F.thumb_batch(COPIES) + [F.image(k) for k in F.ALL[6:]]
    with host.PngEncoder() as cpu:
        want, want64 = cpu.encode(batch), cpu.encode(batch, base64=True)
    assert len({len(w) for w in want[6:6 + COPIES]}) > 10  # the copies differ
    with host.PngEncoder(ctx) as dev:
        same(dev.encode(batch), want, "the mixed batch, numpy through the device")
        tensors = [to_device(a) for a in batch]
        same(dev.encode(tensors), want, "the mixed batch, CUDA tensors")
        same(dev.encode(tensors, base64=True), want64, "the mixed batch, base64")
        same(dev.encode(batch[:3]), want[:3], "a small batch after a large one")  # the encoder's arrays are reused


def scenario_two_encoders(ctx):
    a, b = host.PngEncoder(ctx), host.PngEncoder(ctx)
    x, y = F.image("thumb_noisy"), F.image("gray_127x128")
    wx, wy = host.encode_png(x), host.encode_png(y)
    for _ in range(2):
        same(a.encode([x]), [wx], "the first encoder")
        same(b.encode([y, x]), [wy, wx], "the second encoder")
    a.close()
    same(b.encode([x]), [wx], "the second encoder after the first is closed")
    b.close()


def scenario_refusals(ctx):
    ok = F.image("five_by_three")
    L = host.load()
    with host.PngEncoder(ctx) as e:
        out, offsets = np.full(4096, 0xAB, np.uint8), np.full(4, 7, np.uint64)
        d = to_device(ok)

        def call(n, recs, on_device=1, cap=out.size, handle=None):
            arr = (capi.PngImage * len(recs))(*[capi.PngImage(*r) for r in recs])
            return L.och_png_encoder_encode(e.h if handle is None else handle, n, arr, on_device, 0, out.ctypes.data, cap, offsets.ctypes.data)

        good = (d.data_ptr(), 5, 3, 3, 0)
        # a refused descriptor among valid ones refuses the whole call, and nothing is written
        for bad in ((d.data_ptr(), 5, 3, 2, 0), (d.data_ptr(), 0, 3, 3, 0), (d.data_ptr(), 5, 65536, 3, 0), (None, 5, 3, 3, 0),
                    (d.data_ptr(), 65535, 65535, 4, 0)):
            assert call(3, [good, bad, good]) != 0 and b"image 1" in L.och_png_last_error(), bad
        assert call(2, [good, good], cap=2 * 116 - 1) != 0 and b"add up to" in L.och_png_last_error()
        assert (out == 0xAB).all() and (offsets == 7).all()
        dead = host.PngEncoder(ctx)
        h = dead.h
        dead.close()
        assert call(1, [good], handle=h) != 0 and b"not a live" in L.och_png_last_error()
        assert call(2, [good, good]) == 0
        want = host.encode_png(ok)
        assert bytes(out[:int(offsets[1])]) == want and bytes(out[int(offsets[1]):int(offsets[2])]) == want
        for wrong in (ok.astype(np.float32), np.zeros((4, 4, 2), np.uint8), to_device(ok).to(torch.int16)):
            try:
                e.encode([ok, wrong] if isinstance(wrong, np.ndarray) else [d, wrong])
                raise AssertionError("not refused")
            except ValueError:
                pass


def scenario_graph(ctx):
    """load_images(ctx, thumbnails=True) -> encode_thumbnails(ctx) against the CPU route's text"""
    h, w, f = 240, 320, 300.0
    rng = np.random.default_rng(12)
    y, x = np.mgrid[0:h, 0:w]
    pixels = []
    for i in range(4):
        img = np.zeros((h, w, 3), np.uint8)
        for _ in range(60):
            cy, cx, r = rng.integers(0, h), rng.integers(0, w), rng.integers(4, 20)
            img[(y - cy) ** 2 + (x - cx) ** 2 < r * r] = rng.integers(0, 256, 3)
        pixels.append((img.astype(np.int32) // 2 + ((x + y + 13 * i) % 128)[..., None]).astype(np.uint8))
    pixels = np.stack(pixels)
    model = np.array([f, w / 2, h / 2, 0, 0, 0, 0, 0, w, h], np.float64)
    pos = np.array([(i * 20.0, 3.0 * i, 100.0) for i in range(4)])
    g1, g2 = host.Graph(), host.Graph()
    for g in (g1, g2):
        g.load_images(ctx, pixels, g.add_model(model), pos, max_keypoints=2000, thumbnails=True)
    assert g1.to_json() == g2.to_json()
    assert g1.encode_thumbnails(ctx) == 4 and g2.encode_thumbnails() == 4
    text = g1.to_json()
    assert text == g2.to_json()
    g3 = host.Graph().from_json(text)
    assert g3.decode_thumbnails() == [host.PNG_OK] * 4
    assert sorted(g3.node_ids) == sorted(g1.node_ids)
    for i, nid in enumerate(g1.node_ids):  # a loaded graph orders its nodes by id
        assert np.array_equal(g3.thumbnail(g3.node_ids.index(nid)), g1.thumbnail(i)) and g1.thumbnail(i).std() > 5
    g1.close(), g2.close(), g3.close()


def scenario_mosaic(ctx):
    from PIL import Image

    gsd, t, tile_rows = MOSAIC
    g, s, imgs = four_camera_scene(seed=4)
    plan = mosaic_plan(gsd)
    cfg = dict(tile_size=t, blend_transition_radius=10)
    dimg = [torch.from_numpy(im).to("cuda:0") for im in imgs]
    with host.OrthoMesh(ctx, [s]) as mesh:
        without = []
        plain = host.ortho_mosaic(plan, g, [s], dimg, mesh=mesh, config=cfg, tile_rows=tile_rows, progress=without.append)
        updates = []
        out = host.ortho_mosaic(plan, g, [s], dimg, mesh=mesh, config=cfg, tile_rows=tile_rows, progress=updates.append, progress_png=True)
        assert torch.equal(out, plain) and (plain[..., 3] == 255).any()
        assert all("png_base64" not in u for u in without) and difference(updates, without) == "" and len(updates) >= 4
        cpu = host.PngEncoder()
        for u in updates:
            data = base64.b64decode(u["png_base64"])
            assert np.array_equal(np.asarray(Image.open(io.BytesIO(data))), u["thumbnail"][..., [2, 1, 0, 3]])
            assert cpu.encode([u["thumbnail"]], bgr=True, base64=True)[0] == u["png_base64"]
        cpu.close()
        streamed = []
        out_s = host.ortho_mosaic_streamed(plan, g, [s], lambda i: imgs[i], mesh, len(imgs), config=cfg, tile_rows=tile_rows,
                                           progress=streamed.append, progress_png=True)
        assert torch.equal(out_s, plain) and [u["png_base64"] for u in streamed] == [u["png_base64"] for u in updates]


def scenarios():
    return dict(one_by_one=(scenario_one_by_one,), mixed_batch=(scenario_mixed_batch,), two_encoders=(scenario_two_encoders,),
                refusals=(scenario_refusals,), graph=(scenario_graph,), mosaic=(scenario_mosaic,))


if __name__ == "__main__":
    ctx = capi.Context(0)
    res, device_error = {}, False
    for name, (fn, *args) in scenarios().items():
        try:
            fn(ctx, *args)
            res[name] = "ok"
        except AssertionError:
            res[name] = traceback.format_exc()
        except Exception:  # a device error: nothing more runs on that device
            res[name] = traceback.format_exc()
            device_error = True
            break
    for name in scenarios():
        res.setdefault(name, "not run: an earlier scenario ended in an error")
    print(json.dumps(res), flush=True)
    if not device_error:
        ctx.close()
