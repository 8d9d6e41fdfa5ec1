"""Writes tests/golden/jpeg_texture/: Pillow's (libjpeg-turbo's) baseline 4:2:0 files of the cases jpeg_fixtures.GOLDEN
names, the expected bytes of test_jpeg_host.py.  `python scripts/make_jpeg_golden.py`; needs Pillow."""
import io
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from PIL import Image  # noqa: E402

import jpeg_fixtures as F  # noqa: E402


def pillow_bytes(rgb, quality):
    f = io.BytesIO()
    Image.fromarray(rgb).save(f, format="JPEG", quality=quality, subsampling=2, optimize=False)
    return f.getvalue()


if __name__ == "__main__":
    os.makedirs(F.GOLDEN_DIR, exist_ok=True)
    for case in F.GOLDEN:
        kind, h, w, q, seed = case
        data = pillow_bytes(F.content(kind, h, w, seed), q)
        with open(os.path.join(F.GOLDEN_DIR, F.golden_name(case)), "wb") as f:
            f.write(data)
        print(F.golden_name(case), len(data))
