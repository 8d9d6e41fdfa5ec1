"""The scene and the files of the tests that feed the streamed layered render from JPEG files
(test_ortho_stream_files_host.py, ortho_stream_files_gpu_child.py): the strip scene of
ortho_stream_fixtures with two camera models, its views as baseline JPEG files of this project's encoder, the pixels the
library's own decoder gives for them, and the oriented, unsupported and damaged variants."""
import numpy as np

import jpeg_decode_fixtures as D
from layers_fixtures import DISTORTED
from ortho_fixtures import DOWN, cloud_surface, qmul, quat
from ortho_stream_fixtures import plan_of
from opencalibration_amd import host

AHEAD, LATE = host.LOAD_AHEAD, host.LOAD_LATE
# the second model: 150 x 110, a multiple of neither 16 nor 8 in either axis, 49 500 B an image - no multiple of 256 and
# less than the 57 600 B slot of the 160 x 120 model
SMALL = [94, 75, 55, -0.05, 0.01, 0, 0.001, -0.0005, 150, 110]
TIGHT, ROOMY = 8, 10  # the capacities: the largest band (late loads), two neighbouring bands (ahead loads alone)


def small(i):
    return i % 3 == 1


def two_model_scene(seed=3):
    """strip_scene() with cameras i % 3 == 1 on the 150 x 110 model: 12 cameras in a 6 x 2 layout over a flat mesh, the
    plan 200 x 580 at gsd 0.05 in bands of one 64-pixel tile row, a seeded noise image per camera"""
    rng = np.random.default_rng(seed)
    pos = np.array([(6.0 * x, 5.0 * y, 10.0) for y in range(6) for x in range(2)])
    pos += rng.uniform(-0.4, 0.4, pos.shape) * np.array([1, 1, 0.3])
    ori = [qmul(quat(rng.normal(size=3), 0.04), DOWN) for _ in pos]
    g = host.Graph()
    models = [g.add_model(np.asarray(DISTORTED, np.float64)), g.add_model(np.asarray(SMALL, np.float64))]
    for i, p in enumerate(pos):
        g.add_image(np.zeros((0, 2)), np.zeros(0, np.float32), np.zeros((0, 8), np.uint64), 0, models[small(i)], p)
    g.set_orientations(np.asarray(ori, np.float64).reshape(-1, 4))
    lo, hi = pos[:, :2].min(0) - 6, pos[:, :2].max(0) + 6
    pts = cloud_surface([(lo[0], lo[1], 0), (hi[0], lo[1], 0), (hi[0], hi[1], 0), (lo[0], hi[1], 0),
                         ((lo[0] + hi[0]) / 2, (lo[1] + hi[1]) / 2, 0.5)])
    s = host.rebuild_mesh(pos, previous=pts)
    rng = np.random.default_rng(seed + 1)
    views = [rng.integers(0, 256, (110, 150, 3) if small(i) else (120, 160, 3), dtype=np.uint8) for i in range(len(pos))]
    return g, s, views, plan_of(200, 580, 0.05, -2.0, 27.0), dict(tile_size=64, correspondence_subsample=9)


def with_exif(data, orientation):
    """the file with an APP1 segment of that orientation spliced in behind SOI"""
    payload = D.exif_segment(orientation)
    return data[:2] + b"\xff\xe1" + (len(payload) + 2).to_bytes(2, "big") + payload + data[2:]


_scene = {}


def scene():
    """The scene, made once per process and left unchanged: g, s, plan, cfg, dsm (the CPU route's), files (a JPEG of the CPU
    route's encoder per involved camera), imgs (host.decode_jpeg of each: the yardstick's pixels), hw, sets (per band)."""
    if not _scene:
        g, s, views, plan, cfg = two_model_scene()
        cams = host.ortho_layers_cameras(g, [s])
        assert len(cams["node_ids"]) == len(views)  # every camera is involved, in the graph's order
        files = [host.encode_jpeg(np.ascontiguousarray(v[..., ::-1])) for v in views]
        imgs = [host.decode_jpeg(f) for f in files]
        used = host.ortho_band_cameras(plan, g, [s], config=cfg)
        _scene.update(g=g, s=s, plan=plan, cfg=cfg, files=files, imgs=imgs, hw=cams["image_hw"], dsm=host.dsm_render(plan, [s]),
                      sets=[set(np.nonzero(row)[0].tolist()) for row in used])
        assert all(im.shape[:2] == tuple(hw) for im, hw in zip(imgs, cams["image_hw"]))
    return _scene


def band_dsm(sc, k):
    return sc["dsm"][k * 64:(k + 1) * 64]


def unsupported_file(sc, cam):
    """a file of camera cam's size whose frame header says arithmetic coding"""
    return D.unsupported_by_patch(sc["files"][cam], sc["files"][cam])["arithmetic"]


def corrupt_header_file(sc, cam):
    """camera cam's file cut inside its headers"""
    return sc["files"][cam][:40]


def damaged_scan_file(sc, cam):
    """camera cam's file with bytes of its scan changed so that the headers still parse and the scan does not decode: the
    first such mutation of jpeg_decode_fixtures.damaged, found with the CPU route"""
    for cand in D.damaged(sc["files"][cam], 5, count=40)[9:]:
        if host.jpeg_info(cand)["status"] != "ok":
            continue
        info = host.jpeg_info(cand)
        if (info["height"], info["width"]) != tuple(sc["hw"][cam]):
            continue
        with host.JpegDecoder() as d:
            if d.decode([cand]).status[0] == "corrupt":
                return cand
    raise AssertionError("no mutation left the headers whole and the scan undecodable")


def feed_order(stream):
    """the caller's loop as (band to render, [(band, camera) to load before it]): the band's late loads - all of band 0's -
    then the next band's ahead loads"""
    out = []
    for k in range(stream.num_bands):
        loads = [(k, cam) for cam, _, _ in (stream.loads(k) if k == 0 else stream.loads(k, LATE))]
        if k + 1 < stream.num_bands:
            loads += [(k + 1, cam) for cam, _, _ in stream.loads(k + 1, AHEAD)]
        out.append((k, loads))
    return out


def sweep(stream, how, render):
    """One sweep of the stream.  how(band, cameras): brings those planned loads of `band`; render(k): band k's layers."""
    bands = []
    for k, loads in feed_order(stream):
        for b in sorted({b for b, _ in loads}):
            how(b, [cam for bb, cam in loads if bb == b])
        bands.append(render(k))
    return bands


def by_upload(stream, imgs):
    def how(band, cams):
        for cam in cams:
            stream.upload(band, cam, imgs[cam])
    return how


def by_files(stream, files):
    def how(band, cams):
        if cams:
            assert stream.upload_jpegs(band, cams, [files[c] for c in cams]) == ["ok"] * len(cams)
    return how


def by_both(stream, imgs, files):
    """every band's loads half by upload and half by upload_jpegs, the copies first in even bands and last in odd ones"""
    def how(band, cams):
        copied, decoded = cams[::2], cams[1::2]
        if band % 2:
            by_files(stream, files)(band, decoded)
        by_upload(stream, imgs)(band, copied)
        if not band % 2:
            by_files(stream, files)(band, decoded)
    return how
