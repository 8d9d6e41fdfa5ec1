"""host.GeoCoord against a model of the Transverse Mercator projection that uses no series: in mpmath
at 40 digits, the complex latitude phi_c with psi(phi_c) = psi(phi) + i dlambda (psi: the isometric latitude) is found by
a root search, and the meridian arc is integrated to it; easting = Im, northing = Re minus the arc to latitude_of_origin.
The bound is 1e-7 m: 50 ulp of a 1e7 m northing (one ulp is 1.9e-9 m)."""
import functools
import math
import random

import mpmath as mp
import numpy as np
import pytest

from opencalibration_amd import host

mp.mp.dps = 40
A = mp.mpf(6378137)
F = 1 / mp.mpf("298.257223563")
E2 = F * (2 - F)
E = mp.sqrt(E2)
BOUND = 1e-7


def psi(phi):
    s = mp.sin(phi)
    return mp.atanh(s) - E * mp.atanh(E * s)


def arc(phi):
    """the meridian arc from the equator to the (complex) latitude phi"""
    return A * (1 - E2) * mp.quad(lambda t: (1 - E2 * mp.sin(t) ** 2) ** mp.mpf(-1.5), [0, phi])


def model(lat, lon, lat0, lon0):
    """(easting, northing) in metres, mpmath numbers"""
    phi, dl = mp.radians(mp.mpf(lat)), mp.radians(mp.mpf(lon) - mp.mpf(lon0))
    target = psi(phi) + 1j * dl
    guess = mp.mpc(phi, dl * mp.cos(phi))
    phic = mp.findroot(lambda z: psi(z) - target, guess, tol=mp.mpf(10) ** -35)
    m = arc(phic)
    return mp.im(m), mp.re(m) - arc(mp.radians(mp.mpf(lat0)))


@functools.lru_cache(maxsize=None)
def cases():
    """(geo, lat0r, lon0r, points n x 2, the model's easting / northing of each): computed once"""
    rng = random.Random(31)
    out = []
    for lat0 in (-70.0, -33.9, 0.0, 47.37, 80.0):
        lon0 = round(rng.uniform(-179, 179), 2)            # exact under %g: the centre is the origin
        geo = host.GeoCoord(lat0, lon0)
        assert geo.centre == (lat0, lon0)
        pts = [(lat0 + rng.uniform(-0.5, 0.5), lon0 + rng.uniform(-0.8, 0.8)) for _ in range(12)]
        pts += [(lat0, lon0), (lat0 + 0.5, lon0 - 0.8)]
        ref = [model(la, lo, lat0, lon0) for la, lo in pts]
        out.append((geo, lat0, lon0, np.array(pts), ref))
    return out


def test_forward_against_the_model():
    worst = 0.0
    for geo, lat0, lon0, pts, ref in cases():
        got = geo.to_local(pts[:, 0], pts[:, 1], 12.5)
        assert np.all(got[:, 2] == 12.5)                   # altitude passes through
        for (x, y, _), (ex, ey) in zip(got.tolist(), ref):
            worst = max(worst, abs(float(mp.mpf(x) - ex)), abs(float(mp.mpf(y) - ey)))
    print(f"forward: worst |error| {worst:.3e} m over {sum(len(c[3]) for c in cases())} points")
    assert worst <= BOUND


def test_inverse_against_the_model():
    worst = 0.0
    rng = random.Random(32)
    for geo, lat0, lon0, pts, ref in cases():
        xy = np.array([[rng.uniform(-60000, 60000), rng.uniform(-55000, 55000), 3.0] for _ in range(6)])
        back = geo.to_wgs84(xy)
        assert np.all(back[:, 2] == 3.0)
        for (x, y, _), (lon, lat, _) in zip(xy.tolist(), back.tolist()):
            ex, ey = model(lat, lon, lat0, lon0)
            worst = max(worst, abs(float(ex - mp.mpf(x))), abs(float(ey - mp.mpf(y))))
    print(f"inverse: worst |error| {worst:.3e} m")
    assert worst <= BOUND


def test_round_trip_and_array_shapes():
    geo = host.GeoCoord(47.37, 8.54)
    assert np.array_equal(geo.to_local(47.37, 8.54, 0.0), [0.0, 0.0, 0.0])
    lat, lon = np.full((3, 4), 47.4), np.linspace(8.0, 9.0, 12).reshape(3, 4)
    local = geo.to_local(lat, lon, 100.0)
    assert local.shape == (3, 4, 3)
    back = geo.to_wgs84(local)
    assert back.shape == (3, 4, 3) and np.abs(back[..., 0] - lon).max() < 1e-12 and np.abs(back[..., 1] - lat).max() < 1e-12
    assert geo.to_local([], [], []).shape == (0, 3) and geo.to_wgs84(np.zeros((0, 3))).shape == (0, 3)
    assert local[0, 0, 0] < 0 < local[2, 3, 0] and np.all(local[..., 1] > 0)        # east is +x, north is +y


@pytest.mark.parametrize("lat, lon, lat_text, lon_text", [(47.376912, 151.234567, "47.3769", "151.235"),
                                                          (-33.912345, -70.6543219, "-33.9123", "-70.6543"),
                                                          (0.00001234567, 8.5, "1.23457e-05", "8.5")])
def test_the_origin_is_kept_and_the_centre_is_percent_g_of_it(lat, lon, lat_text, lon_text):
    geo = host.GeoCoord(lat, lon)
    assert geo.origin == (lat, lon)                                                 # getOriginLatitude(): unrounded
    assert geo.centre == (float(lat_text), float(lon_text)) == (float("%g" % lat), float("%g" % lon))
    assert np.array_equal(geo.to_local(*geo.centre, 5.0), [0.0, 0.0, 5.0])          # the projection is about the rounded pair
    off = geo.to_local(lat, lon, 0.0)
    if geo.centre != geo.origin:
        assert 0 < math.hypot(off[0], off[1]) < 60
    ex, ey = model(lat, lon, *geo.centre)
    assert abs(off[0] - float(ex)) <= BOUND and abs(off[1] - float(ey)) <= BOUND
    wkt = geo.wkt()
    assert wkt.startswith('PROJCS["Custom Transverse Mercator",\n    GEOGCS["WGS 84",\n        DATUM["WGS_1984",\n'
                          '            SPHEROID["WGS 84",6378137,298.257223563,\n')
    assert ('    PROJECTION["Transverse_Mercator"],\n    PARAMETER["latitude_of_origin",%s],\n    PARAMETER["central_meridian",%s],\n'
            '    PARAMETER["scale_factor",1],\n    PARAMETER["false_easting",0],\n    PARAMETER["false_northing",0],\n'
            '    UNIT["metre",1,\n        AUTHORITY["EPSG","9001"]],\n    AXIS["Easting",EAST],\n    AXIS["Northing",NORTH]]'
            % (lat_text, lon_text)) in wkt and wkt.endswith("NORTH]]")


def test_what_cannot_be_transformed_is_three_nans():
    geo = host.GeoCoord(10.0, 20.0)
    nan, inf = float("nan"), float("inf")
    bad = geo.to_local([nan, 10, 10, inf, 10, 10, 91, 10], [20, nan, 20, 20, 110, -70, 20, 20 + 90], [0, 0, nan, 0, 0, 0, 0, 0])
    assert np.all(np.isnan(bad))
    ok = geo.to_local([10, 10], [109.9, -69.9], [0, 0])                             # just inside 90 degrees
    assert np.all(np.isfinite(ok))
    assert np.all(np.isnan(geo.to_wgs84([[nan, 0, 0], [0, inf, 0], [0, 0, nan], [1e9, 0, 0]])))
    wrapped = host.GeoCoord(0.0, 179.5).to_local(0.0, -179.5, 0.0)                  # one degree east, across the date line
    assert 110000 < wrapped[0] < 112000
    for lat, lon in ((nan, 0.0), (0.0, inf), (95.0, 0.0)):
        with pytest.raises(ValueError):
            host.GeoCoord(lat, lon)
