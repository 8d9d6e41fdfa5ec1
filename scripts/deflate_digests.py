"""SHA-256 and length of what the host route of the two DEFLATE codecs writes for the tests' fixtures: every image of
png_fixtures.ALL in both channel orders (one batch each), every raster of geotiff_fixtures.RGBA and the dsm as whole files
(geo tags, overview levels, sparse off), and the five crafted payloads through deflate_tiles.  The streams are a function of
the pixels alone, so a change of the encoder that leaves behaviour alone leaves every digest alone.

  python scripts/deflate_digests.py            compare with tests/golden/deflate/parent_digests.json, exit 1 on a difference
  python scripts/deflate_digests.py --write    write that file (run at the commit whose bytes are to be kept)

tests/test_deflate_digests.py asserts the comparison.  Needs no GPU."""
import hashlib
import io
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
GOLDEN = os.path.join(ROOT, "tests", "golden", "deflate", "parent_digests.json")


def _entry(data):
    return dict(sha256=hashlib.sha256(data).hexdigest(), bytes=len(data))


def digests():
    import geotiff_fixtures as G
    import png_fixtures as F
    from opencalibration_amd import host

    out = {}
    with host.PngEncoder() as e:
        for bgr in (False, True):
            files = e.encode([F.image(k) for k in F.ALL], bgr=bgr)
            for k, data in zip(F.ALL, files):
                out[f"png/{k}/{'bgr' if bgr else 'rgb'}"] = _entry(data)
    for name in G.RGBA + ("dsm",):
        f = io.BytesIO()
        host.save_geotiff(f, G.dsm() if name == "dsm" else G.rgba(name), geo=G.GEO, sparse=False)
        out[f"geotiff/{name}"] = _entry(f.getvalue())
    names, payloads = G.crafted()
    for k, stream in zip(names, host.deflate_tiles(payloads)):
        out[f"crafted/{k}"] = _entry(stream)
    return out


def main():
    got = digests()
    if "--write" in sys.argv:
        os.makedirs(os.path.dirname(GOLDEN), exist_ok=True)
        with open(GOLDEN, "w") as f:
            json.dump(got, f, indent=1, sort_keys=True)
            f.write("\n")
        print(f"{len(got)} digests written to {GOLDEN}")
        return 0
    with open(GOLDEN) as f:
        want = json.load(f)
    bad = sorted(k for k in set(want) | set(got) if want.get(k) != got.get(k))
    for k in bad:
        print(f"{k}: {want.get(k)} -> {got.get(k)}")
    print(f"{len(got) - len(bad)} of {len(want)} digests as stored")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
