"""The streamed layered render on the host (csrc/host/ortho_stream.cpp, ortho_residency.hpp, ortho_layers.cpp): the CPU
route of the bands' camera sets against the per-band union of the CPU render's own kNN lists; the subset render against
the full-table render, bit for bit; the residency plan against a Python restatement of its rule and a simulator of its
invariants; and the stream object's ordering contract on its CPU route (slots in host memory)."""
import numpy as np
import pytest

from ortho_stream_fixtures import (AHEAD, BAND_SET_SCENES, LATE, band_cameras_raw, knn_band_sets, knn_offer_sets, plan_restated,
                                   scene_overflow, sets_of, simulate, strip_scene, used_of)
from opencalibration_amd import capi, host


def same_layers(a, b):
    assert np.array_equal(a["bgra"], b["bgra"])
    assert np.array_equal(a["camera_id"], b["camera_id"])
    assert np.array_equal(a["weight"].view(np.uint32), b["weight"].view(np.uint32))
    assert a["correspondences"].tobytes() == b["correspondences"].tobytes()


# ---- band sets ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(BAND_SET_SCENES))
def test_band_sets_equal_the_union_of_the_renders_knn(name):
    g, s, imgs, plan, cfg = BAND_SET_SCENES[name]()
    dsm = np.zeros((plan["height"], plan["width"]), np.float32)
    full = host.ortho_layers(plan, g, [s], imgs, config=cfg, dsm=dsm, debug_knn=True)
    expected = knn_band_sets(full["knn"], len(imgs), cfg["tile_size"])
    got = host.ortho_band_cameras(plan, g, [s], tile_rows=1, config=cfg)
    assert got.shape == expected.shape and np.array_equal(got, expected)
    assert expected.any(1).all()
    if name == "four_cameras":
        assert (full["knn"] == 0xFFFFFFFF).any() and expected.all()
    else:
        assert not expected.all()  # the sets differ from band to band
    two = host.ortho_band_cameras(plan, g, [s], tile_rows=2, config=cfg)
    assert np.array_equal(two, knn_band_sets(full["knn"], len(imgs), 2 * cfg["tile_size"]))
    g.close()


def test_band_sets_of_the_overflow_scene_against_the_knn_restated():
    """1 030 coincident cameras: every pixel's list is decided by ties, which numpy's sort does not order as knn_offer does"""
    cams, plan = scene_overflow()
    expected = knn_offer_sets(cams, plan, 16)
    assert np.array_equal(band_cameras_raw(cams, plan, 16), expected)
    assert expected.any(1).all() and not expected.all()


# ---- subset render -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def strip():
    g, s, imgs, plan, cfg = strip_scene()
    dsm = host.dsm_render(plan, [s])
    used = host.ortho_band_cameras(plan, g, [s], config=cfg)
    yield dict(g=g, s=s, imgs=imgs, plan=plan, cfg=cfg, dsm=dsm, used=used)
    g.close()


@pytest.fixture(scope="module")
def strip_full_bands(strip):
    t = strip["cfg"]["tile_size"]
    return [host.ortho_layers(strip["plan"], strip["g"], [strip["s"]], strip["imgs"], row0=row0, tile_rows=1, config=strip["cfg"],
                              dsm=strip["dsm"][row0:row0 + t], debug_knn=True) for row0 in range(0, strip["plan"]["height"], t)]


def test_subset_render_equals_full_render(strip, strip_full_bands):
    t, n = strip["cfg"]["tile_size"], len(strip["imgs"])
    proper = 0
    for k, full in enumerate(strip_full_bands):
        own = np.nonzero(strip["used"][k])[0]
        subsets = [own]
        if len(own) < n:
            proper += 1
            extra = [c for c in range(n) if c not in own]
            subsets.append(np.sort(np.append(own, extra[k % len(extra)])))
        for sub in subsets:
            part = host.ortho_layers(strip["plan"], strip["g"], [strip["s"]], [strip["imgs"][i] for i in sub], row0=k * t,
                                     tile_rows=1, config=strip["cfg"], dsm=strip["dsm"][k * t:(k + 1) * t], debug_knn=True,
                                     subset=sub)
            same_layers(part, full)
            assert np.array_equal(part["knn"], full["knn"])
    assert proper >= 3 and (strip_full_bands[0]["bgra"][..., 3] == 255).any()
    assert sum(len(b["correspondences"]) for b in strip_full_bands) > 0


def test_subset_render_equals_full_render_on_the_exact_tie_scene():
    """the lattice's ties are broken by camera order, which a subset keeps"""
    g, s, imgs, plan, cfg = BAND_SET_SCENES["exact_ties"]()
    used = host.ortho_band_cameras(plan, g, [s], config=cfg)
    dsm = np.zeros((plan["height"], plan["width"]), np.float32)
    for k in range(len(used)):
        sub = np.nonzero(used[k])[0]
        args = dict(row0=16 * k, tile_rows=1, config=cfg, dsm=dsm[16 * k:16 * k + 16], debug_knn=True)
        full = host.ortho_layers(plan, g, [s], imgs, **args)
        part = host.ortho_layers(plan, g, [s], [imgs[i] for i in sub], subset=sub, **args)
        same_layers(part, full)
        assert np.array_equal(part["knn"], full["knn"])
    g.close()


@pytest.mark.parametrize("subset", [[1, 0, 2, 3, 4], [0, 1, 1, 2, 3], [0, 1, 2, 3, 12]])
def test_subset_render_refuses_a_bad_subset(strip, subset):
    with pytest.raises(capi.OchipError, match="subset entry"):
        host.ortho_layers(strip["plan"], strip["g"], [strip["s"]], strip["imgs"][:5], row0=0, tile_rows=1, config=strip["cfg"],
                          dsm=strip["dsm"][:64], subset=subset)


# ---- the plan ---------------------------------------------------------------------------------------------------------------
def check(sets, n_cams, capacity, resident=None):
    loads, state = host.ortho_residency_plan(used_of(sets, n_cams), capacity, resident)
    expected, expected_state = plan_restated(sets, capacity, resident)
    assert loads == expected
    assert state.tolist() == expected_state
    return loads, simulate(sets, capacity, loads, resident), state


def test_plan_equals_the_restated_rule_on_random_sets():
    rng = np.random.default_rng(2024)
    late = 0
    for _ in range(200):
        n_bands, n_cams = int(rng.integers(1, 13)), int(rng.integers(1, 41))
        sets = [set(rng.choice(n_cams, int(rng.integers(0, min(n_cams, 9) + 1)), replace=False).tolist()) for _ in range(n_bands)]
        biggest = max(1, max(len(s) for s in sets))
        capacity = biggest + int(rng.integers(0, 5))
        loads, _, state = check(sets, n_cams, capacity)
        late += sum(l[2] == LATE for band in loads for l in band)
        check(sets, n_cams, capacity, state.tolist())  # a second sweep from the state the first one left
    assert late > 0


def windows(n_bands, width, step):
    return [set(range(k * step, k * step + width)) for k in range(n_bands)]


def test_sliding_windows_with_room_for_two_bands_load_every_camera_once_ahead():
    sets = windows(8, 6, 2)
    capacity = max(len(a | b) for a, b in zip(sets, sets[1:]))
    loads, count, _ = check(sets, 6 + 7 * 2, capacity)
    assert all(l[2] == AHEAD for band in loads for l in band)
    assert count == {c: 1 for c in range(6 + 7 * 2)}


def test_capacity_of_the_largest_band_needs_late_loads():
    sets = windows(8, 6, 2)
    loads, count, _ = check(sets, 20, 6)
    assert any(l[2] == LATE for band in loads for l in band)
    assert count == {c: 1 for c in range(20)}


def test_a_camera_that_leaves_and_returns_under_a_small_capacity_is_loaded_twice():
    sets = [{0, 1}, {2, 3}, {0, 4}]
    _, count, _ = check(sets, 5, 2)
    assert count[0] == 2
    _, count, _ = check(sets, 5, 5)
    assert count[0] == 1  # with room it stays


def test_a_band_larger_than_the_capacity_is_refused_with_the_band_named():
    sets = [{0}, {1, 2}, {0, 1, 2, 3}, {1}]
    with pytest.raises(capi.OchipError, match=r"band 2 reads 4 images, the capacity is 3"):
        host.ortho_residency_plan(used_of(sets, 4), 3)


def test_empty_sets_and_a_single_band():
    loads, _, state = check([set(), {1, 2}, set(), {2, 3}], 4, 2)
    assert loads[0] == [] and loads[2] == []
    loads, _, _ = check([{3, 1}], 4, 2)
    assert loads == [[(1, 0, AHEAD), (3, 1, AHEAD)]]
    loads, _, _ = check([set()], 4, 1)
    assert loads == [[]]
    loads, state = host.ortho_residency_plan(np.zeros((0, 4), bool), 2)
    assert loads == [] and state.tolist() == [-1, -1]


# ---- the stream object, CPU route -------------------------------------------------------------------------------------------
def drive(stream, imgs, sweep_check=None):
    """the caller's loop: late loads of band k, ahead loads of band k + 1, render(k)"""
    bands = []
    for k in range(stream.num_bands):
        for cam, _, _ in (stream.loads(k) if k == 0 else stream.loads(k, LATE)):
            stream.upload(k, cam, imgs[cam])
        if k + 1 < stream.num_bands:
            for cam, _, _ in stream.loads(k + 1, AHEAD):
                stream.upload(k + 1, cam, imgs[cam])
        bands.append(stream.render(k, dsm=sweep_check["dsm"][k * 64:(k + 1) * 64]))
    return bands


@pytest.mark.parametrize("tight", [False, True])
def test_cpu_stream_equals_the_full_render_over_two_sweeps(strip, strip_full_bands, tight):
    sets = sets_of(strip["used"])
    capacity = max(len(s) for s in sets) if tight else max(len(a | b) for a, b in zip(sets, sets[1:]))
    assert capacity < len(strip["imgs"])
    with host.OrthoStream(strip["plan"], strip["g"], [strip["s"]], capacity, config=strip["cfg"]) as stream:
        assert stream.num_bands == len(sets)
        assert [set(stream.band_cameras(k).tolist()) for k in range(stream.num_bands)] == sets
        planned = [stream.loads(k) for k in range(stream.num_bands)]
        expected, state = plan_restated(sets, capacity)
        assert planned == expected
        assert any(l[2] == LATE for band in planned for l in band) == tight
        for sweep in range(2):
            for got, full in zip(drive(stream, strip["imgs"], strip), strip_full_bands):
                same_layers(got, full)
            if sweep == 0:
                stream.rewind()
                again = [stream.loads(k) for k in range(stream.num_bands)]
                assert again == plan_restated(sets, capacity, state)[0] and again != planned


def test_cpu_stream_refuses_calls_out_of_the_plans_order(strip):
    sets = sets_of(strip["used"])
    capacity = max(len(a | b) for a, b in zip(sets, sets[1:]))
    imgs = strip["imgs"]
    with pytest.raises(capi.OchipError, match=r"band \d+ reads \d+ images, the capacity is 2"):
        host.OrthoStream(strip["plan"], strip["g"], [strip["s"]], 2, config=strip["cfg"])
    with host.OrthoStream(strip["plan"], strip["g"], [strip["s"]], capacity, config=strip["cfg"]) as stream:
        with pytest.raises(capi.OchipError, match="not uploaded"):
            stream.render(0, dsm=strip["dsm"][:64])
        with pytest.raises(capi.OchipError, match="ascending"):
            stream.render(1, dsm=strip["dsm"][64:128])
        k = next(k for k in range(2, stream.num_bands) if stream.loads(k))
        cam = stream.loads(k)[0][0]
        with pytest.raises(capi.OchipError, match=rf"waits for render\({k - 2}\)"):
            stream.upload(k, cam, imgs[cam])
        with pytest.raises(capi.OchipError, match="no planned load"):
            stream.upload(0, next(c for c in range(len(imgs)) if c not in sets[0]), imgs[0])
        with pytest.raises(capi.OchipError, match="rewind"):
            stream.rewind()
        first = stream.loads(0)[0][0]
        stream.upload(0, first, imgs[first])
        with pytest.raises(capi.OchipError, match="uploaded already"):
            stream.upload(0, first, imgs[first])
        with pytest.raises(ValueError):
            stream.upload(0, stream.loads(0)[1][0], imgs[0][:10])
    tight = max(len(s) for s in sets)
    with host.OrthoStream(strip["plan"], strip["g"], [strip["s"]], tight, config=strip["cfg"]) as stream:
        k, cam = next((k, l[0]) for k in range(1, stream.num_bands) for l in stream.loads(k, LATE))
        if k >= 2:  # an ahead load would be accepted here, a late one is not
            for j in range(k - 1):
                for c, _, _ in stream.loads(j):
                    stream.upload(j, c, imgs[c])
                stream.render(j, dsm=strip["dsm"][j * 64:(j + 1) * 64])
        with pytest.raises(capi.OchipError, match=rf"late load .* waits for render\({k - 1}\)"):
            stream.upload(k, cam, imgs[cam])
