"""The averaged overview levels on the CPU route (csrc/host/ortho_overview.cpp, csrc/ortho_overview.hpp)
against the rule restated in numpy, level by level from the level before: uint8 levels equal, float32 levels equal bit for
bit.  Every shape with every content, the builder fed in band partitions against the whole raster in one feed, and the
refusals."""
import numpy as np
import pytest

from opencalibration_amd import capi, host
from ortho_overviews_fixtures import (PARTITION_SHAPE, PARTITIONS, SHAPES, cases, fed_in_bands, raster, restated, same)


@pytest.mark.parametrize("shape", sorted(SHAPES), ids=lambda s: f"{s[0]}x{s[1]}")
def test_level_sizes(shape):
    w, h = shape
    assert host.overview_levels(w, h) == [(lh, lw) for lw, lh in SHAPES[shape]]
    assert [(l.shape[1], l.shape[0]) for l in restated(np.zeros((h, w), np.float32))] == SHAPES[shape]


@pytest.mark.parametrize("name,content,w,h", cases(), ids=[c[0] for c in cases()])
def test_cpu_route_equals_restatement(name, content, w, h):
    level0 = raster(content, w, h)
    got, want = host.ortho_overviews(level0), restated(level0)
    assert len(got) == len(want) == len(SHAPES[(w, h)])
    for k, (g, x) in enumerate(zip(got, want)):
        assert same(g, x), (k + 1, int((g != x).sum()))


def test_contents_reach_the_cases_they_are_for():
    w, h = 129, 200
    three = raster("three_of_four_255", w, h)
    valid = np.zeros((h + h % 2, w + w % 2), int)
    valid[:h, :w] = three[..., 3] > 0
    cells = valid[0::2, 0::2] + valid[0::2, 1::2] + valid[1::2, 0::2] + valid[1::2, 1::2]
    assert (cells[:h // 2, :w // 2] == 3).all()
    assert (restated(three)[0][:h // 2, :w // 2, :3] == 255).all()  # (3 * 255 + 1) // 3
    lone = restated(raster("one_valid", w, h))
    assert all((l[..., 3] > 0).sum() == 1 for l in lone[:3])  # an averaged alpha of 64, 16, 4 still counts as valid
    big = raster("large_halves", w, h)
    planes = [np.nan_to_num(big[i:h - 1 + i:2, j:w - 1 + j:2]) for i in (0, 1) for j in (0, 1)]
    f32 = (planes[0] + planes[1] + planes[2] + planes[3]).astype(np.float32)
    f64 = sum(p.astype(np.float64) for p in planes)
    assert (f32.astype(np.float64) != f64).any()  # a float sum rounds where the double sum does not
    assert np.isnan(restated(raster("nan_but_one", w, h))[0]).sum() == 65 * 100 - 2


@pytest.mark.parametrize("content", ["alpha_mixed", "nan_random", "large_halves"])
@pytest.mark.parametrize("partition", sorted(PARTITIONS))
def test_band_partitions_equal_the_whole_raster(content, partition):
    w, h = PARTITION_SHAPE
    level0 = raster(content, w, h)
    assert sum(PARTITIONS[partition]) == h
    got, want = fed_in_bands(host, level0, PARTITIONS[partition]), host.ortho_overviews(level0)
    assert len(got) == 7
    for k, (g, x) in enumerate(zip(got, want)):
        assert same(g, x), (partition, k + 1)


def test_bgra_is_served_by_the_same_rule():
    level0 = raster("alpha_mixed", 65, 65)
    swapped = np.ascontiguousarray(level0[..., [2, 1, 0, 3]])
    for a, b in zip(host.ortho_overviews(level0), host.ortho_overviews(swapped)):
        assert np.array_equal(a[..., [2, 1, 0, 3]], b)


def test_zero_levels_is_valid():
    for w, h in ((1, 1), (2, 2), (2, 9)):
        assert host.ortho_overviews(raster("alpha_255", w, h)) == []
        with host.OrthoOverviews(host.OVERVIEW_FLOAT32, w, h) as b:
            b.feed(0, raster("nan_random", w, h))
            assert b.complete_rows(1) == 0
            assert b.finish() == []


def test_refusals_name_the_rows():
    level0 = raster("alpha_half", 20, 30)

    def builder():
        return host.OrthoOverviews(host.OVERVIEW_RGBA8, 20, 30)

    with builder() as b:  # a gap
        b.feed(0, level0[0:10])
        with pytest.raises(capi.OchipError, match=r"gap: rows 12 to 20 .* row 10 is next"):
            b.feed(12, level0[12:20])
        b.feed(10, level0[10:30])  # a refused feed changes nothing
        assert all(same(g, x) for g, x in zip(b.finish(), restated(level0)))
    with builder() as b:  # an overlap
        b.feed(0, level0[0:10])
        with pytest.raises(capi.OchipError, match=r"overlap: rows 8 to 16 .* row 10 is next"):
            b.feed(8, level0[8:16])
    with builder() as b:  # the first band does not start at row 0
        with pytest.raises(capi.OchipError, match=r"gap: rows 1 to 5 .* row 0 is next"):
            b.feed(1, level0[1:5])
    with builder() as b:  # beyond the raster
        b.feed(0, level0[0:20])
        with pytest.raises(capi.OchipError, match=r"rows 20 to 31 .* 30 rows"):
            b.feed(20, np.concatenate([level0[20:30], level0[:1]]))
    with builder() as b:  # finish before the last row
        b.feed(0, level0[0:29])
        with pytest.raises(capi.OchipError, match=r"finish before the last row: rows 0 to 29 of 30"):
            b.finish()
        b.feed(29, level0[29:30])
        b.finish()
        with pytest.raises(capi.OchipError, match=r"rows 30 to 31 after finish"):  # a feed after finish
            b.feed(30, level0[:1])
    L = host.load()
    assert L.och_ortho_overviews_feed(None, 0, 1, None) == -1  # OCHIP_EINVAL
    with builder() as b:
        assert L.och_ortho_overviews_feed(b.h, 3, 4, level0.ctypes.data) == -1
        assert b"gap" in L.och_ortho_overviews_last_error()


def test_bad_arguments():
    with pytest.raises(ValueError):
        host.ortho_overviews(np.zeros((4, 4, 3), np.uint8))
    with pytest.raises(ValueError):
        host.ortho_overviews(np.zeros((4, 4), np.float64))
    with pytest.raises(ValueError):
        host.overview_levels(0, 5)
    with pytest.raises(ValueError):
        host.OrthoOverviews(host.OVERVIEW_RGBA8, 8, 8, on_device=True)  # device levels without a context
    with pytest.raises(ValueError):
        host.OrthoOverviews(host.OVERVIEW_RGBA8, 8, 8, levels=[np.zeros((4, 4, 4), np.uint8)])  # 8 x 8 has two levels
    with host.OrthoOverviews(host.OVERVIEW_RGBA8, 8, 8) as b:
        with pytest.raises(ValueError):
            b.feed(0, np.zeros((8, 8), np.float32))
