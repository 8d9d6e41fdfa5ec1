"""Graph.load_survey's refusals need no device: every one comes from the files' bytes, before a context is
looked at, names the file and leaves the graph as it was.  A survey that passes them asks for the context."""
import importlib.util
import os

import numpy as np
import pytest

from opencalibration_amd import capi, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SURVEY_DIR = os.path.join(ROOT, "tests", "golden", "survey_files")


def path(name):
    return os.path.join(SURVEY_DIR, name + ".jpg")


@pytest.mark.parametrize("name, text", [("no_app1", "has no latitude / longitude"), ("zero_denominator", None),
                                        ("xmp_before_exif", None), ("le_north_east_35mm", None)])
def test_the_committed_files(name, text):
    g = host.Graph()
    with pytest.raises(capi.OchipError) as e:
        g.load_survey(None, [path("le_inch"), path(name)])
    if text is None:                       # a good survey: only the context is missing
        assert "needs a device context" in str(e.value)
    else:
        assert text in str(e.value) and f"file 1 ({path(name)})" in str(e.value)
    assert g.num_nodes == 0 and g.geo is None and len(g.models()) == 0


def test_each_refusal_names_the_file():
    spec = importlib.util.spec_from_file_location("make_survey_golden", os.path.join(ROOT, "scripts", "make_survey_golden.py"))
    S = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(S)
    plain, gps = S.base_jpeg(), S.gps_ifd(47.0, 8.0, S.R(100, 1))
    size = {0xa002: S.W, 0xa003: S.H}
    whole = S.splice(plain, [S.exif_bytes({0x010f: "Acme"}, {**size, 0xa405: 30}, gps)])
    bad = [(S.splice(plain, [S.exif_bytes({0x010f: "Acme"}, {**size, 0xa405: 30})]), "file 1 has no latitude / longitude"),
           (S.splice(plain, [S.exif_bytes({0x010f: "Acme"}, size, gps)]), "file 1 has no focal length"),
           (S.splice(plain, [S.exif_bytes({0x010f: "Acme"}, {0xa405: 30}, gps)]), "file 1 has no image size"),
           (S.splice(plain, [S.exif_bytes({0x010f: "Acme"}, {0xa002: S.W + 1, 0xa003: S.H, 0xa405: 30}, gps)]),
            f"file 1 decodes to {S.W} x {S.H}, its metadata says {S.W + 1} x {S.H}"),
           (S.splice(plain, [S.exif_bytes({0x010f: "Acme", 0x0112: 6}, {**size, 0xa405: 30}, gps)]),   # turned by its orientation
            f"file 1 decodes to {S.H} x {S.W}, its metadata says {S.W} x {S.H}"),
           (whole[:whole.index(b"\xff\xdb") + 3], "file 1 is corrupt")]
    g = host.Graph()
    g.add_image(np.zeros((1, 2)), np.ones(1, np.float32), np.zeros((1, 8), np.uint64), 1, g.add_model([100, 32, 24, 0, 0, 0, 0, 0, 64, 48]),
                (0, 0, 0))
    before = g.to_json()
    for data, text in bad:
        with pytest.raises(capi.OchipError) as e:
            g.load_survey(None, [whole, data, whole])
        assert text in str(e.value), (text, str(e.value))
        assert g.to_json() == before and g.geo is None and len(g.models()) == 1
    with pytest.raises(capi.OchipError) as e:
        g.load_survey(None, [whole, whole])
    assert "needs a device context" in str(e.value) and g.to_json() == before and g.geo is None
