"""The bytes of the host route of both DEFLATE codecs (csrc/deflate_rules.hpp under host/geotiff.cpp and host/png.cpp) against
the digests stored when the two encoders became one (tests/golden/deflate/parent_digests.json, scripts/deflate_digests.py):
every PNG fixture in both channel orders, every GeoTIFF fixture and the dsm as whole files, the crafted payloads' streams.
The GPU tests assert device == host route byte for byte, so together they pin the device's bytes too.  Needs no GPU."""
import importlib.util
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("deflate_digests", os.path.join(ROOT, "scripts", "deflate_digests.py"))
deflate_digests = importlib.util.module_from_spec(spec)
spec.loader.exec_module(deflate_digests)


def test_host_route_bytes_are_the_stored_ones():
    with open(deflate_digests.GOLDEN) as f:
        want = json.load(f)
    got = deflate_digests.digests()
    assert len(want) == 2 * 19 + 8 + 5
    assert sorted(got) == sorted(want)
    assert {k: v for k, v in got.items() if want[k] != v} == {}
