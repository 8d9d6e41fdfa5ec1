"""Writes tests/golden/jpeg_decode/: the small .jpg inputs Pillow's encoder makes (jpeg_decode_fixtures.PILLOW_GOLDEN and
EXIF_GOLDEN), copies of sample files given with --samples DIR, and expected.json with the pixels Pillow (libjpeg-turbo)
decodes from them and from tests/golden/jpeg_texture/*.jpg - as <name>.bgr beside the input, or as a SHA-256 where that
would exceed 64 KB.  `python scripts/make_jpeg_decode_golden.py [--samples DIR]`; needs Pillow."""
import json
import os
import shutil
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import jpeg_decode_fixtures as D  # noqa: E402
import jpeg_fixtures as F  # noqa: E402


def main():
    os.makedirs(D.GOLDEN_DIR, exist_ok=True)
    for name, kind, h, w, seed, sampling, quality, options in D.PILLOW_GOLDEN:
        with open(os.path.join(D.GOLDEN_DIR, name + ".jpg"), "wb") as f:
            f.write(D.pillow_encode(F.content(kind, h, w, seed), sampling, quality, **options))
    for name, orientation, big_endian in D.EXIF_GOLDEN:
        with open(os.path.join(D.GOLDEN_DIR, name + ".jpg"), "wb") as f:
            f.write(D.exif_file(orientation, big_endian, name == D.EXIF_THUMBNAIL_FIXTURE))
    if "--samples" in sys.argv:
        src = sys.argv[sys.argv.index("--samples") + 1]
        for s in D.REFERENCE_SAMPLES:
            shutil.copyfile(os.path.join(src, s), os.path.join(D.GOLDEN_DIR, "sample_" + s))
    expected, stored = {}, {}  # stored: the SHA-256 of pixels already written -> their file, so equal pixels are kept once
    for name, path in sorted(D.golden_files().items()):
        data = open(path, "rb").read()
        assert len(data) <= D.MAX_FIXTURE_BYTES, name
        entry = {}
        for key, apply in (("oriented", True), ("plain", False)):
            px = D.pillow_decode(data, apply)
            e = {"shape": list(px.shape)}
            if px.size <= D.MAX_FIXTURE_BYTES:
                digest = D.sha256(px)
                if digest not in stored:
                    stored[digest] = f"{name}.{key}.bgr"
                    px.tofile(os.path.join(D.GOLDEN_DIR, stored[digest]))
                e["file"] = stored[digest]
            else:
                e["sha256"] = D.sha256(px)
            entry[key] = e
        expected[name] = entry
    with open(D.MANIFEST, "w") as f:
        json.dump(expected, f, indent=1, sort_keys=True)
        f.write("\n")
    print(len(expected), "files")


if __name__ == "__main__":
    main()
