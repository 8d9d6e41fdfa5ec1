"""The restatement of the extract stage's working image (oracle.gray_resize: oracle/akaze.cpp, bgr_to_gray + area_table +
resize_area) held against the float64 model of tests/working_image_fixtures.py - the definitions of the grey conversion and
of area resampling, with which it shares no code - under the comparison rule stated there, on every case the device test
(tests/test_gpu_working_image.py) runs.  Also: the cap on the band of undecidable pixels on the model alone, every mutation
of the model seen, the restated dispatch reaching every route, and the byte-split dot products of the fused grey conversion
over all 2^24 BGR codes.  No device.

WORKING_IMAGE_FIGURES (pytest -s): per case the working size, the largest tap counts, delta, the band's share of the pixels
and the restatement's worst |got - m| outside the band (at most 0.5 - delta when every such pixel is rounded right).
  case                 working    taps     delta     band     worst outside (restatement = device, bit-equal)
  4000x100             1600 x 40  3 x 3    3.04e-04  0.000 %  0.484512   (also -primaries 0.483418, -blobs 0.484954)
  4376x100             1600 x 37  4 x 4    3.65e-04  0.086 %  0.499607
  4380x100             1600 x 37  4 x 4    3.65e-04  0.079 %  0.499619
  1604x100             1600 x 100 2 x 2    2.43e-04  0.046 %  0.499754
  1601x3               1600 x 3   2 x 2    2.43e-04  0.042 %  0.499612
  3200x96              1600 x 48  2 x 2    0         none     0.5 (ties, compared)
  40x3200              20 x 1600  2 x 2    0         none     0.5
  400x5004             128 x 1600 5 x 5    4.26e-04  0.080 %  0.499572
  2002x100             1600 x 80  3 x 3    3.04e-04  0.050 %  0.499690   (-primaries: 0.062 %, 0.499693)
  6400x64              1600 x 16  4 x 4    0         none     0.5
  12000x100            1600 x 13  8 x 8    6.08e-04  0.091 %  0.499332
  16000x100            1600 x 10  10 x 10  7.30e-04  0.281 %  0.499253
  33x21, 64x64         unresized  1 x 1    0         none     0
No pixel outside the band is rounded wrong in any case; inside it the restatement is off the model's rounding by one level
in a handful of pixels (4376, 4380, 1604, 2002-primaries).  Mutations, pixels wrong outside the band / worst levels:
rgb_weights 60511 of 64000 / 30, g_r_exchanged 61661 of 64000 / 45, half_up_general 787 of 25600 (6400x64) and 834 of 32000
(40x3200) / 1, even_in_vector_body 9605 of 76800 / 1, slivers_kept 234 of 4800 (1601x3) / 1, last_cell_full 1599 of 160000
/ 57 (the last row of 1604x100), box_taps all / 93.

Findings.  The restatement and the model agree everywhere, so neither was changed.  The case list differs from the sizes
first proposed in three places, each from the restated dispatch and confirmed by the route the device reports: 400 x 5000
has 4 horizontal taps, not 5 (s = 3.125: footprints start at multiples of 1/8 and a fifth tap would be a sliver), so the
fused-8 case is 400 x 5004; widths 4364 - 4372 do not stage although 4376 does (the window limit is not monotone), which
leaves 4376 / 4380 as the pair either side of the limit; and dropping the sliver rule moves no pixel at 1604 (its slivers
are of the order 1e-5 of a pixel), so 1601 x 3 was added, where a sliver of 0.000625 of a white row decides 5 % of the
pixels."""
import numpy as np
import pytest

import working_image_fixtures as wf


@pytest.fixture(scope="module")
def models():
    """Image, model and restated working image per case: computed once, never written to."""
    cache = {}

    def get(name, oracle):
        if name not in cache:
            img, model = wf.built(name)
            got = oracle.gray_resize(img, model.W, model.H)
            got.setflags(write=False)
            cache[name] = (img, model, got)
        return cache[name]

    return get


@pytest.mark.parametrize("case", wf.CASES, ids=repr)
def test_restatement_against_the_model(case, models, oracle):
    img, model, got = models(case.name, oracle)
    f = wf.check(got, model)
    print(f"WORKING_IMAGE_FIGURES {case.name}: {model.W} x {model.H}, taps {model.tx} x {model.ty}, delta {model.delta:.2e}, "
          f"band {100 * f['band_share']:.3f} %, worst outside {f['worst_outside']:.6f}, wrong outside {f['wrong_outside']}, "
          f"worst levels {f['worst_levels']}")
    assert f["band_share"] <= wf.BAND_CAP          # the condition on the input, from the model alone
    assert wf.passed(f), f


@pytest.mark.parametrize("case", wf.CASES, ids=repr)
def test_the_band_cap_holds_on_the_model_alone(case):
    model = wf.built(case.name)[1]
    assert model.band_share <= wf.BAND_CAP, model.band_share
    assert 0.0 <= model.delta < 2e-3
    if model.resized and model.s not in (2.0, 4.0, 8.0):
        assert model.delta > 5e-5


@pytest.mark.parametrize("mutation", wf.MUTATIONS)
def test_every_mutation_is_seen(mutation, models, oracle):
    assert wf.MUTATION_CASES[mutation]
    for name in wf.MUTATION_CASES[mutation]:
        img, model, got = models(name, oracle)
        assert wf.passed(wf.check(got, model))
        f = wf.check(got, wf.Model(img, mutation))
        print(f"WORKING_IMAGE_FIGURES mutation {mutation} on {name}: wrong outside {f['wrong_outside']} of {f['pixels']}, "
              f"worst levels {f['worst_levels']}")
        assert not wf.passed(f)
        assert wf.mutation_seen(f), (mutation, name, f)


def test_the_restated_dispatch_reaches_every_route():
    seen_resize, seen_grey = set(), set()
    for case in wf.CASES:
        model = wf.built(case.name)[1]
        assert wf.routes(model, aligned=True) == (case.resize, case.grey), (case.name, wf.routes(model))
        seen_resize.add(case.resize), seen_grey.add(case.grey)
        for _ in case.offsets:
            r, g = wf.routes(model, aligned=False)
            assert g == wf.GREY_BYTEWISE and r in (wf.RESIZE_NONE, wf.RESIZE_STAGED_GREY, wf.RESIZE_PER_TAP)
            seen_resize.add(r), seen_grey.add(g)
    assert seen_resize == set(range(5)) and seen_grey == set(range(4))
    # what the cases are there for
    taps = {c.name: wf.built(c.name)[1] for c in wf.CASES if c.kind == "noise"}
    assert (taps["4000x100"].tx, taps["4376x100"].tx, taps["4380x100"].tx) == (3, 4, 4)
    assert taps["400x5004"].tx == 5 and taps["12000x100"].tx == 8 and taps["16000x100"].tx > 8
    assert (taps["4000x100"].W, taps["4000x100"].H) == (1600, 40) and taps["4000x100"].s != 2.5
    assert (taps["40x3200"].W, taps["40x3200"].H) == (20, 1600) and taps["3200x96"].W % 16 == 0
    assert taps["6400x64"].s == 4.0 and taps["3200x96"].s == 2.0


def test_the_byte_split_dot_products_are_the_grey_conversion():
    """The fused route computes a pixel's grey from its three bytes in one dword with two 4 x 8-bit dot products, the 14-bit
    weights split into bytes: 1868 = 7 * 256 + 76, 9617 = 37 * 256 + 145, 4899 = 19 * 256 + 35, the high parts packed as
    0x00132507 and the low ones as 0x0023914C (the fourth byte meets a zero weight): hi = dot(p, 0x00132507), grey =
    (dot(p, 0x0023914C) + (hi << 8) + 2^13) >> 14, in 32-bit unsigned arithmetic.  All 2^24 BGR codes, and a fourth byte
    of any value."""
    assert (7 * 256 + 76, 37 * 256 + 145, 19 * 256 + 35) == (1868, 9617, 4899)
    code = np.arange(1 << 24, dtype=np.uint32)

    def udot4(a, b, acc):
        out = acc.astype(np.uint32)
        for k in range(4):
            out = out + ((a >> np.uint32(8 * k)) & np.uint32(255)) * np.uint32((b >> (8 * k)) & 255)
        return out

    b, g, r = (code & 255).astype(np.int64), ((code >> 8) & 255).astype(np.int64), ((code >> 16) & 255).astype(np.int64)
    want = (1868 * b + 9617 * g + 4899 * r + (1 << 13)) >> 14
    for top in (0, 0xA5, 0xFF):
        p = code | np.uint32(top << 24)
        hi = udot4(p, 0x00132507, np.zeros(1, np.uint32))
        got = udot4(p, 0x0023914C, (hi << np.uint32(8)) + np.uint32(1 << 13)) >> np.uint32(14)
        assert np.array_equal(got.astype(np.int64), want)
    assert want.max() == 255 and want.min() == 0
