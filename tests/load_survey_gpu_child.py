"""The scenarios of test_gpu_load_survey.py in one process with one capi.Context(0) (torch comes up before libochip.so).
`python load_survey_gpu_child.py <tests dir> <repo dir>` prints one JSON line: {scenario: "ok" | the traceback}."""
import contextlib
import importlib.util
import json
import os
import sys
import tempfile
import traceback

import numpy as np
import torch  # noqa: F401

if __name__ == "__main__":
    sys.path[:0] = sys.argv[1:3]

from opencalibration_amd import capi, host  # noqa: E402

ORIGIN = (47.376912, 8.541694)
ORDER = "AABBABAA"
SIZE = dict(A=(320, 240), B=(256, 192))


def golden_script(repo):
    spec = importlib.util.spec_from_file_location("make_survey_golden", os.path.join(repo, "scripts", "make_survey_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@contextlib.contextmanager
def raises(text):
    try:
        yield
    except capi.OchipError as e:
        assert text in str(e), str(e)
    else:
        raise AssertionError(f"no error with {text!r}")


def picture(w, h, seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    img = np.zeros((h, w, 3), np.uint8)
    for _ in range(60):  # bright and dark discs on a gradient: corners for the detector
        cy, cx, r = rng.integers(0, h), rng.integers(0, w), rng.integers(4, 20)
        img[(y - cy) ** 2 + (x - cx) ** 2 < r * r] = rng.integers(0, 256, 3)
    return (img.astype(np.int32) // 2 + ((x + y + 13 * seed) % 128)[..., None]).astype(np.uint8)


def survey(S):
    """the eight files: camera A (DJI, XMP) and camera B (plain GPS), a few tens of metres apart"""
    files = []
    for i, cam in enumerate(ORDER):
        w, h = SIZE[cam]
        lat, lon = ORIGIN[0] + 0.00018 * (i % 4), ORIGIN[1] + 0.0003 * (i // 4) + 0.00002 * i
        size = {0xa002: w, 0xa003: h}
        if cam == "A":
            dji = dict(S.DJI)
            dji.update({"drone-dji:RelativeAltitude": "+%.2f" % (80 + i), "drone-dji:CalibratedFocalLength": "310.5"})
            segs = [S.exif_bytes({0x010f: "DJI", 0x0110: "FC-A"}, size, S.gps_ifd(lat, lon, S.R(5000 + i, 10))), S.xmp_packet(dji)]
        else:
            segs = [S.exif_bytes({0x010f: "Acme", 0x0110: "B-cam"}, {**size, 0xa405: 30}, S.gps_ifd(lat, lon, S.R(900 + i, 10)),
                                 big_endian=True)]
        files.append(S.splice(host.encode_jpeg(picture(w, h, i)), segs))
    return files


def scenario_load_survey(ctx, S, tmp):
    files = survey(S)
    paths = []
    for i, data in enumerate(files):  # every other file goes in as a path
        p = os.path.join(tmp, f"img_{i}.jpg")
        with open(p, "wb") as f:
            f.write(data)
        paths.append(p if i % 2 == 0 else data)
    g1 = host.Graph()
    means = g1.load_survey(ctx, paths, max_keypoints=2000, thumbnails=True, chunk=2)

    # the same by hand: Pillow's reading, GeoCoord, one load_jpegs per run
    md = [S.pillow_metadata(d)[0] for d in files]
    geo = host.GeoCoord(md[0]["capture_info"]["latitude"], md[0]["capture_info"]["longitude"])
    assert g1.geo.origin == geo.origin and g1.geo.centre == geo.centre
    g2, model_of, sums = host.Graph(), {}, np.zeros(2)
    for cam in "AB":
        c = md[ORDER.index(cam)]["camera_info"]
        w, h = c["dimensions"]
        assert (w, h) == SIZE[cam]
        model_of[cam] = g2.add_model([c["focal_length_px"], w / 2, h / 2, 0, 0, 0, 0, 0, w, h])
    pos = np.array([geo.to_local(m["capture_info"]["latitude"], m["capture_info"]["longitude"], m["capture_info"]["altitude"]) for m in md])
    assert 10 < np.linalg.norm(pos[1, :2] - pos[0, :2]) < 100 and pos[0, 2] == 80.0   # the relative altitude
    for a, b in ((0, 2), (2, 4), (4, 5), (5, 6), (6, 8)):
        f, s = g2.load_jpegs(ctx, files[a:b], model_of[ORDER[a]], pos[a:b], max_keypoints=2000, thumbnails=True, chunk=2)
        sums += (f * (b - a), s * (b - a))
    assert g1.num_nodes == g2.num_nodes == 8 and g1.node_ids == g2.node_ids
    assert np.array_equal(np.array(means), sums / 8) and means[0] > 0
    assert np.array_equal(g1.models(), g2.models()) and len(g1.models()) == 2
    assert np.array_equal(g1.node_table()["model"], g2.node_table()["model"])
    assert list(g1.node_table()["model"]) == [0, 0, 1, 1, 0, 1, 0, 0]
    for i in range(8):
        a, b = g1.node_payload(i), g2.node_payload(i)
        for k in ("loc", "strength", "desc", "position"):
            assert np.array_equal(a[k], b[k]), (i, k)
        assert np.array_equal(a["position"], pos[i])
        assert np.array_equal(g1.thumbnail(i), g2.thumbnail(i)) and g1.thumbnail(i) is not None
        assert a["path"] == (paths[i] if i % 2 == 0 else b["path"])
        assert json.dumps(g1.node_metadata(i)) == json.dumps(md[i])   # NaN-safe: the same text

    # paths and metadata survive a checkpoint
    cp = os.path.join(tmp, "checkpoint")
    host.save_checkpoint(cp, g1, origin=g1.geo.origin)
    g3, _, meta = host.load_checkpoint(cp)
    assert meta["origin"] == g1.geo.origin                                  # unrounded
    back = {int(i): k for k, i in enumerate(g3.node_table()["id"])}
    for i, nid in enumerate(g1.node_ids):
        assert g3.node_payload(back[nid])["path"] == g1.node_payload(i)["path"]
        assert json.dumps(g3.node_metadata(back[nid])) == json.dumps(md[i])

    # link, then the GeoJSON
    g1.link(ctx)
    doc = json.loads(g1.to_geojson())
    kinds = [f["geometry"]["type"] for f in doc["features"]]
    assert kinds.count("Point") == 8 and kinds.count("LineString") == g1.num_edges
    lon, lat, alt = doc["features"][kinds.index("Point")]["geometry"]["coordinates"]
    assert abs(lat - ORIGIN[0]) < 0.01 and abs(lon - ORIGIN[1]) < 0.01
    want = sorted(e["n_inliers"] for e in g1.edges())
    assert sorted(f["properties"]["inliers"] for f in doc["features"] if f["geometry"]["type"] == "LineString") == want

    # a second survey into the same graph keeps the frame and the models
    g1.load_survey(ctx, files[:2], max_keypoints=2000)
    assert g1.num_nodes == 10 and len(g1.models()) == 2 and g1.geo.origin == geo.origin
    for g in (g1, g2, g3):
        g.close()


def scenario_refusals(ctx, S, tmp):
    files = survey(S)[:3]
    w, h = SIZE["A"]
    size = {0xa002: w, 0xa003: h}
    plain = host.encode_jpeg(picture(w, h, 40))
    gps = S.gps_ifd(47.0, 8.0, S.R(100, 1))
    bad = dict(
        no_position=(S.splice(plain, [S.exif_bytes({0x010f: "Acme"}, {**size, 0xa405: 30})]), "has no latitude / longitude"),
        no_focal=(S.splice(plain, [S.exif_bytes({0x010f: "Acme"}, size, gps)]), "has no focal length"),
        no_size=(S.splice(plain, [S.exif_bytes({0x010f: "Acme"}, {0xa405: 30}, gps)]), "has no image size"),
        other_size=(S.splice(plain, [S.exif_bytes({0x010f: "Acme"}, {0xa002: w + 1, 0xa003: h, 0xa405: 30}, gps)]), "its metadata says"),
        turned=(S.splice(plain, [S.exif_bytes({0x010f: "Acme", 0x0112: 6}, {**size, 0xa405: 30}, gps)]), "its metadata says"),
        no_metadata=(plain, "has no latitude / longitude"),
    )
    whole = S.splice(plain, [S.exif_bytes({0x010f: "Acme"}, {**size, 0xa405: 30}, gps)])
    bad["cut_in_its_headers"] = (whole[:whole.index(b"\xff\xdb") + 3], "is corrupt")   # the metadata reads, the decoder's parse ends
    g = host.Graph()
    g.load_survey(ctx, files[:1], max_keypoints=2000)
    before, geo = g.to_json(), g.geo
    for name, (data, text) in bad.items():
        with raises(text):                                                   # refused before a context is looked at
            g.load_survey(None, [files[1], data], max_keypoints=2000)
        p = os.path.join(tmp, name + ".jpg")
        with open(p, "wb") as f:
            f.write(data)
        with raises(text):
            g.load_survey(ctx, [files[1], data, files[2]], max_keypoints=2000)
        with raises(p):                                                      # a path is named
            g.load_survey(ctx, [files[1], p], max_keypoints=2000)
        assert g.num_nodes == 1 and g.to_json() == before and g.geo is geo and len(g.models()) == 1, name
    fresh = host.Graph()
    with raises("file 0"):
        fresh.load_survey(ctx, [bad["no_focal"][0]])
    assert fresh.geo is None and fresh.num_nodes == 0 and len(fresh.models()) == 0
    g.load_survey(ctx, files[1:], max_keypoints=2000)                        # and the graph still loads
    assert g.num_nodes == 3
    g.close(), fresh.close()


SCENARIOS = dict(load_survey=scenario_load_survey, refusals=scenario_refusals)


if __name__ == "__main__":
    S = golden_script(sys.argv[2])
    ctx = capi.Context(0)
    res, device_error = {}, False
    with tempfile.TemporaryDirectory(prefix="load_survey_") as tmp:
        for name, fn in SCENARIOS.items():
            try:
                fn(ctx, S, tmp)
                res[name] = "ok"
            except AssertionError:
                res[name] = traceback.format_exc()
            except Exception:  # a device error: nothing more runs on that device
                res[name] = traceback.format_exc()
                device_error = True
                break
    for name in SCENARIOS:
        res.setdefault(name, "not run: an earlier scenario ended in an error")
    print(json.dumps(res), flush=True)
    if not device_error:
        ctx.close()
