"""The streamed layered render fed from JPEG files, on the CPU route (csrc/host/ortho_stream.cpp's
och_ortho_stream_upload_jpegs, host.OrthoStream.upload_jpegs, ortho_mosaic_streamed(files=...)).
The yardstick everywhere is the route that existed before: the same stream fed through upload() with host.decode_jpeg's
pixels of the same files.  Every comparison is bit for bit: BGRA, camera ids, weights and correspondences per band, RGBA for
mosaics.  The refusals launch nothing and mark nothing, which the tests show by the next render being refused with the
band's full count and the stream then completing correctly through upload().  The host sources run once more under the
address and undefined-behaviour sanitizers in a stand-alone program (tests/ortho_stream_files_driver.cpp)."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import ortho_stream_files_fixtures as X
from opencalibration_amd import capi, host


def same_layers(a, b):
    assert np.array_equal(a["bgra"], b["bgra"])
    assert np.array_equal(a["camera_id"], b["camera_id"])
    assert np.array_equal(a["weight"].view(np.uint32), b["weight"].view(np.uint32))
    assert a["correspondences"].tobytes() == b["correspondences"].tobytes()


@pytest.fixture(scope="module")
def sc():
    return X.scene()


def open_stream(sc, capacity):
    return host.OrthoStream(sc["plan"], sc["g"], [sc["s"]], capacity, config=sc["cfg"])


def two_sweeps(sc, capacity, how_of):
    """the bands of two sweeps of a fresh stream, fed by how_of(stream)"""
    with open_stream(sc, capacity) as stream:
        render = lambda k: stream.render(k, dsm=X.band_dsm(sc, k))  # noqa: E731
        first = X.sweep(stream, how_of(stream), render)
        stream.rewind()
        return first + X.sweep(stream, how_of(stream), render)


@pytest.fixture(scope="module")
def yardstick(sc):
    """capacity -> the bands of two sweeps through upload() of the decoded pixels: computed once, left unchanged"""
    out = {c: two_sweeps(sc, c, lambda st: X.by_upload(st, sc["imgs"])) for c in (X.TIGHT, X.ROOMY)}
    assert (out[X.TIGHT][0]["bgra"][..., 3] == 255).any() and sum(len(b["correspondences"]) for b in out[X.TIGHT]) > 0
    return out


def test_the_scene_is_the_one_the_cases_need(sc):
    assert [len(s) for s in sc["sets"]] == [6, 6, 8, 8, 8, 8, 8, 6, 6, 6]
    assert sorted({tuple(hw) for hw in sc["hw"].tolist()}) == [(110, 150), (120, 160)]
    with open_stream(sc, X.TIGHT) as stream:
        loads = [stream.loads(k) for k in range(stream.num_bands)]
    assert [k for k, b in enumerate(loads) if any(l[2] == X.LATE for l in b)] == [4, 5]
    assert [k for k, b in enumerate(loads) if any(l[2] == X.AHEAD for l in b)] == [0, 2]
    assert any([l[1] for l in b] != sorted(l[1] for l in b) or b[0][1] > 0 for b in loads if b)  # scattered slots
    assert any({X.small(l[0]) for l in b} == {False, True} for b in loads)  # one call decodes both image sizes
    with open_stream(sc, X.ROOMY) as stream:
        assert all(l[2] == X.AHEAD for k in range(stream.num_bands) for l in stream.loads(k))


@pytest.mark.parametrize("capacity", [X.TIGHT, X.ROOMY])
def test_upload_jpegs_equals_upload_over_two_sweeps(sc, yardstick, capacity):
    got = two_sweeps(sc, capacity, lambda st: X.by_files(st, sc["files"]))
    assert len(got) == 2 * len(sc["sets"])
    for a, b in zip(got, yardstick[capacity]):
        same_layers(a, b)


@pytest.mark.parametrize("capacity", [X.TIGHT, X.ROOMY])
def test_a_band_fed_half_by_upload_and_half_by_upload_jpegs(sc, yardstick, capacity):
    for a, b in zip(two_sweeps(sc, capacity, lambda st: X.by_both(st, sc["imgs"], sc["files"])), yardstick[capacity]):
        same_layers(a, b)


def test_a_file_with_orientation_3_is_decoded_as_its_oriented_pixels(sc):
    cam = 4  # a 150 x 110 camera: the half turn keeps the size
    assert X.small(cam)
    files, imgs = list(sc["files"]), list(sc["imgs"])
    files[cam] = X.with_exif(files[cam], 3)
    assert host.jpeg_info(files[cam])["orientation"] == 3
    imgs[cam] = host.decode_jpeg(files[cam])
    assert np.array_equal(imgs[cam], sc["imgs"][cam][::-1, ::-1]) and not np.array_equal(imgs[cam], sc["imgs"][cam])
    for a, b in zip(two_sweeps(sc, X.TIGHT, lambda st: X.by_files(st, files)), two_sweeps(sc, X.TIGHT, lambda st: X.by_upload(st, imgs))):
        same_layers(a, b)


@pytest.fixture(scope="module")
def mosaics(sc):
    """color_balance -> the mosaic through fetch= alone"""
    return {cb: host.ortho_mosaic_streamed(sc["plan"], sc["g"], [sc["s"]], lambda i: sc["imgs"][i], None, X.TIGHT, config=sc["cfg"],
                                           color_balance=cb) for cb in (None, "solve")}


@pytest.mark.parametrize("color_balance", [None, "solve"])
def test_mosaic_from_files_equals_mosaic_from_fetch(sc, mosaics, color_balance):
    got = host.ortho_mosaic_streamed(sc["plan"], sc["g"], [sc["s"]], None, None, X.TIGHT, config=sc["cfg"], color_balance=color_balance,
                                     files=sc["files"])
    assert np.array_equal(got, mosaics[color_balance]) and (got[..., 3] == 255).any()
    assert color_balance is None or not np.array_equal(got, mosaics[None])


def test_mosaic_from_paths(sc, mosaics, tmp_path):
    paths = []
    for i, f in enumerate(sc["files"]):
        paths.append(tmp_path / f"{i}.jpg")
        paths[-1].write_bytes(f)
    got = host.ortho_mosaic_streamed(sc["plan"], sc["g"], [sc["s"]], None, None, X.ROOMY, config=sc["cfg"], files=paths)
    assert np.array_equal(got, mosaics[None])


def test_mosaic_falls_back_to_fetch_for_cameras_without_a_usable_file(sc, mosaics):
    files = list(sc["files"])
    files[2], files[7] = None, X.unsupported_file(sc, 7)
    fetched = []

    def fetch(i):
        fetched.append(i)
        return sc["imgs"][i]

    got = host.ortho_mosaic_streamed(sc["plan"], sc["g"], [sc["s"]], fetch, None, X.TIGHT, config=sc["cfg"], files=files)
    assert np.array_equal(got, mosaics[None]) and sorted(set(fetched)) == [2, 7]
    # without fetch: refused with the camera and the status named, before the band that reads the camera renders
    rendered = []
    original = host.OrthoStream.render

    def spy(self, band, *a, **k):
        rendered.append(band)
        return original(self, band, *a, **k)

    host.OrthoStream.render = spy
    try:
        with pytest.raises(capi.OchipError, match=r"camera 7 .*unsupported"):
            host.ortho_mosaic_streamed(sc["plan"], sc["g"], [sc["s"]], None, None, X.TIGHT, config=sc["cfg"], files=files)
        first_band_of_7 = min(k for k, s in enumerate(sc["sets"]) if 7 in s)
        assert all(k < first_band_of_7 for k in rendered)
        rendered.clear()
        files[7] = sc["files"][7]
        with pytest.raises(capi.OchipError, match=r"camera 2 has no file"):
            host.ortho_mosaic_streamed(sc["plan"], sc["g"], [sc["s"]], None, None, X.TIGHT, config=sc["cfg"], files=files)
        assert all(k < min(k for k, s in enumerate(sc["sets"]) if 2 in s) for k in rendered)
    finally:
        host.OrthoStream.render = original


# ---- refusals -----------------------------------------------------------------------------------------------------------
def refused_and_nothing_marked(sc, yardstick, band, call, match, prepare=0):
    """A stream brought through `prepare` bands by upload(); call(stream) is refused with `match`; the render of `band` is
    then refused with the band's full count of loads still pending - the refused call marked none - and the stream
    completes through upload() with the yardstick's bands."""
    imgs = sc["imgs"]
    with open_stream(sc, X.TIGHT) as stream:
        order = X.feed_order(stream)
        bands = []
        done = set()
        for k, loads in order[:prepare]:
            for b, cam in loads:
                stream.upload(b, cam, imgs[cam])
                done.add((b, cam))
            bands.append(stream.render(k, dsm=X.band_dsm(sc, k)))
        with pytest.raises(capi.OchipError, match=match):
            call(stream)
        missing = len([1 for cam, _, _ in stream.loads(band) if (band, cam) not in done])
        assert missing > 0
        # the bands before `band` complete through upload(), its own loads wait until its render has been refused
        held = []
        for k, loads in order[prepare:]:
            held += [(b, cam) for b, cam in loads if b == band and (b, cam) not in done]
            if k == band:
                assert len(held) == missing
                with pytest.raises(capi.OchipError, match=rf"render: {missing} planned loads of band {band} are not uploaded"):
                    stream.render(band, dsm=X.band_dsm(sc, band))
            for b, cam in loads + (held if k == band else []):
                if (b, cam) not in done and (b != band or k == band):
                    stream.upload(b, cam, imgs[cam])
                    done.add((b, cam))
            bands.append(stream.render(k, dsm=X.band_dsm(sc, k)))
        for a, b in zip(bands, yardstick[X.TIGHT]):
            same_layers(a, b)


def band0(sc):
    """band 0's planned loads at the tight capacity: cameras 6 .. 11, two of them (7, 10) on the small model"""
    return [6, 7, 8, 9, 10, 11]


def test_refused_an_unplanned_camera(sc, yardstick):
    files = sc["files"]
    refused_and_nothing_marked(sc, yardstick, 0, lambda st: st.upload_jpegs(0, [6, 7, 0], [files[6], files[7], files[0]]),
                               "camera 0 is no planned load of band 0")


def test_refused_the_same_camera_twice(sc, yardstick):
    files = sc["files"]
    refused_and_nothing_marked(sc, yardstick, 0, lambda st: st.upload_jpegs(0, [6, 7, 6], [files[6], files[7], files[6]]),
                               "camera 6 appears twice")


def test_refused_a_camera_already_uploaded(sc, yardstick):
    files, imgs = sc["files"], sc["imgs"]
    with open_stream(sc, X.TIGHT) as stream:
        stream.upload(0, 6, imgs[6])
        with pytest.raises(capi.OchipError, match="camera 6 of band 0 is uploaded already"):
            stream.upload_jpegs(0, [7, 6], [files[7], files[6]])
        with pytest.raises(capi.OchipError, match="render: 5 planned loads of band 0 are not uploaded"):
            stream.render(0, dsm=X.band_dsm(sc, 0))
        assert stream.upload_jpegs(0, [7, 8, 9, 10, 11], [files[c] for c in (7, 8, 9, 10, 11)]) == ["ok"] * 5
        same_layers(stream.render(0, dsm=X.band_dsm(sc, 0)), yardstick[X.TIGHT][0])


def test_refused_an_ahead_load_before_its_band_is_due(sc, yardstick):
    files = sc["files"]
    # band 2's ahead loads (cameras 4 and 5) wait for render(0)
    refused_and_nothing_marked(sc, yardstick, 2, lambda st: st.upload_jpegs(2, [4, 5], [files[4], files[5]]),
                               r"ahead load of camera 4 for band 2 waits for render\(0\)")


def test_refused_a_late_load_before_its_band_is_due(sc, yardstick):
    files = sc["files"]
    # band 4's late loads (cameras 2 and 3) wait for render(3); two bands are rendered
    refused_and_nothing_marked(sc, yardstick, 4, lambda st: st.upload_jpegs(4, [2, 3], [files[2], files[3]]),
                               r"late load of camera 2 for band 4 waits for render\(3\)", prepare=2)


def test_refused_a_null_file(sc, yardstick):
    files = sc["files"]
    refused_and_nothing_marked(sc, yardstick, 0, lambda st: st.upload_jpegs(0, [6, 7], [files[6], None]), "camera 7 has no file")


def header_refusal(sc, yardstick, cam, bad, match, status):
    """band 0's six files in one call, camera `cam`'s replaced by `bad`: refused as a whole, info filled"""
    def call(stream):
        try:
            stream.upload_jpegs(0, band0(sc), [bad if c == cam else sc["files"][c] for c in band0(sc)])
        finally:
            assert stream.jpeg_status == [status if c == cam else "ok" for c in band0(sc)]
    refused_and_nothing_marked(sc, yardstick, 0, call, match)


def test_refused_an_unsupported_header(sc, yardstick):
    header_refusal(sc, yardstick, 10, X.unsupported_file(sc, 10), "file of camera 10 is unsupported", "unsupported")


def test_refused_a_corrupt_header(sc, yardstick):
    header_refusal(sc, yardstick, 8, X.corrupt_header_file(sc, 8), "file of camera 8 is corrupt", "corrupt")


def test_refused_a_file_of_the_other_cameras_size(sc, yardstick):
    header_refusal(sc, yardstick, 7, sc["files"][6], r"file of camera 7 decodes to 160 x 120, the camera's images are 150 x 110", "ok")


def test_refused_a_file_whose_orientation_swaps_its_size(sc, yardstick):
    turned = X.with_exif(sc["files"][7], 6)
    info = host.jpeg_info(turned)
    assert (info["width"], info["height"], info["status"]) == (110, 150, "ok")
    assert host.decode_jpeg(turned).shape == (150, 110, 3)  # and it decodes
    header_refusal(sc, yardstick, 7, turned, r"file of camera 7 decodes to 110 x 150, the camera's images are 150 x 110", "ok")


def test_no_files_is_accepted_and_does_nothing(sc):
    with open_stream(sc, X.TIGHT) as stream:
        assert stream.upload_jpegs(0, [], []) == []
        with pytest.raises(capi.OchipError, match="render: 6 planned loads of band 0"):
            stream.render(0, dsm=X.band_dsm(sc, 0))


def test_a_damaged_scan_leaves_its_load_pending_and_the_others_count(sc, yardstick):
    """CPU route only: no damaged scan is ever fed to a kernel"""
    cam = 10
    bad = X.damaged_scan_file(sc, cam)
    with open_stream(sc, X.TIGHT) as stream:
        with pytest.raises(capi.OchipError, match=rf"scan of the file of camera {cam} is corrupt"):
            stream.upload_jpegs(0, band0(sc), [bad if c == cam else sc["files"][c] for c in band0(sc)])
        assert stream.jpeg_status == ["corrupt" if c == cam else "ok" for c in band0(sc)]
        with pytest.raises(capi.OchipError, match="render: 1 planned loads of band 0 are not uploaded"):
            stream.render(0, dsm=X.band_dsm(sc, 0))
        with pytest.raises(capi.OchipError, match="camera 6 of band 0 is uploaded already"):
            stream.upload(0, 6, sc["imgs"][6])
        stream.upload(0, cam, sc["imgs"][cam])
        same_layers(stream.render(0, dsm=X.band_dsm(sc, 0)), yardstick[X.TIGHT][0])


def test_mosaic_fetches_the_pixels_of_a_scan_that_turns_out_corrupt(sc, mosaics):
    files = list(sc["files"])
    files[10] = X.damaged_scan_file(sc, 10)
    fetched = []

    def fetch(i):
        fetched.append(i)
        return sc["imgs"][i]

    got = host.ortho_mosaic_streamed(sc["plan"], sc["g"], [sc["s"]], fetch, None, X.ROOMY, config=sc["cfg"], files=files)
    assert np.array_equal(got, mosaics[None]) and fetched == [10]
    with pytest.raises(capi.OchipError, match="scan of the file of camera 10 is corrupt"):
        host.ortho_mosaic_streamed(sc["plan"], sc["g"], [sc["s"]], None, None, X.ROOMY, config=sc["cfg"], files=files)


def test_ortho_image_paths_follow_set_node_path(sc):
    g = sc["g"]
    ids = host.ortho_layers_cameras(g, [sc["s"]])["node_ids"]
    index_of = {nid: i for i, nid in enumerate(g.node_ids)}
    try:
        for j, nid in enumerate(ids):
            g.set_node_path(index_of[int(nid)], f"/survey/DJI_{int(nid) % 1000:04d}_{j}.JPG")
        paths = host.ortho_image_paths(g, [sc["s"]])
        assert paths == [f"/survey/DJI_{int(nid) % 1000:04d}_{j}.JPG" for j, nid in enumerate(ids)]
        assert paths == [g.node_payload(index_of[int(nid)])["path"] for nid in ids]
    finally:
        for i in range(len(g.node_ids)):
            g.set_node_path(i, "")


# ---- the stand-alone program under the sanitizers ---------------------------------------------------------------------
def test_scattered_offsets_in_the_stand_alone_program_under_the_sanitizers(sc):
    """tests/ortho_stream_files_driver.cpp: band 0's and band 4's files of the tight plan decoded through
    och_jpeg_decoder_decode's offsets into a heap block of exactly capacity x slot bytes, every file in a heap block of
    exactly its size, with the header refusals and the damaged scan among them; the slots it reports equal the pixels of
    host.decode_jpeg, the slots it must not touch keep their fill."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    d = tempfile.mkdtemp(prefix="ortho_stream_files_driver_")
    exe = os.path.join(d, "driver")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-DOCHIP_JPEG_DECODE_STANDALONE", "-I", os.path.join(root, "include"), "-o", exe,
           os.path.join(root, "tests", "ortho_stream_files_driver.cpp"),
           os.path.join(root, "opencalibration_amd", "csrc", "host", "jpeg_decode.cpp")]
    if subprocess.run(cmd + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True).returncode != 0:
        subprocess.run(cmd, check=True)  # where the sanitizers' runtime does not link
    slot_bytes = 120 * 160 * 3
    with open_stream(sc, X.TIGHT) as stream:
        calls = [stream.loads(0), stream.loads(4)[::-1] + stream.loads(2)]  # slots 0 .. 5, then 5, 4, 6, 7: not ascending
    variants = {7: X.damaged_scan_file(sc, 7), 9: X.unsupported_file(sc, 9), 3: X.corrupt_header_file(sc, 3)}
    lines, expect = [], []
    for c, loads in enumerate(calls):
        for cam, slot, _ in loads:
            data = variants.get(cam, sc["files"][cam])
            path = os.path.join(d, f"{c}_{cam}.jpg")
            with open(path, "wb") as f:
                f.write(data)
            h, w = sc["hw"][cam]
            lines.append(f"{c} {slot} {w} {h} {path}")
            expect.append((c, cam, slot, "ok" if cam not in variants else {7: "corrupt", 9: "unsupported", 3: "corrupt"}[cam]))
    with open(os.path.join(d, "list.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    r = subprocess.run([exe, os.path.join(d, "list.txt"), str(X.TIGHT), str(slot_bytes), os.path.join(d, "slots.bin")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    rows = r.stdout.strip().splitlines()
    assert [row.split() for row in rows if row[0] != "#"] == [[str(c), str(slot), st] for c, _, slot, st in expect], r.stdout
    assert "# refused: a slot outside the block" in rows and "# refused: a NULL file" in rows
    # the block replayed: the driver's fill (0xA5), then every decoded image at its slot in the order of the calls; a refused
    # file and a corrupt scan write nothing, and nothing is written behind an image's last byte
    want = np.full(X.TIGHT * slot_bytes, 0xA5, np.uint8)
    for c, cam, slot, st in expect:
        if st == "ok":
            want[slot * slot_bytes:slot * slot_bytes + sc["imgs"][cam].size] = sc["imgs"][cam].ravel()
    assert {st for _, _, _, st in expect} == {"ok", "unsupported", "corrupt"}
    assert np.array_equal(np.fromfile(os.path.join(d, "slots.bin"), np.uint8), want)
