"""Writes tests/golden/survey_files/: small JPEGs (64 x 48) whose EXIF / XMP cover what host.jpeg_metadata reads, and
expected.json with the metadata Pillow's own reader returns from each, mapped as the reference's extract_metadata maps its
reader's fields.  Pillow only.  Run from the repository root: python scripts/make_survey_golden.py"""
import io
import json
import math
import os
import re
import struct

from PIL import Image
from PIL.TiffImagePlugin import IFDRational as R

XMP_ID = b"http://ns.adobe.com/xap/1.0/\0"
W, H = 64, 48


def base_jpeg(width=W, height=H, seed=1, quality=85):
    """a plain baseline JPEG (JFIF only) of a smooth pattern"""
    px = bytes((3 * x + 5 * y + 40 * c + seed) % 256 for y in range(height) for x in range(width) for c in range(3))
    out = io.BytesIO()
    Image.frombytes("RGB", (width, height), px).save(out, "JPEG", quality=quality)
    return out.getvalue()


def app1(payload):
    assert len(payload) + 2 < 65536
    return b"\xff\xe1" + struct.pack(">H", len(payload) + 2) + payload


def splice(jpeg, segments):
    """the APP1 segments right after SOI, in the given order"""
    assert jpeg[:2] == b"\xff\xd8"
    return jpeg[:2] + b"".join(app1(s) for s in segments) + jpeg[2:]


def exif_bytes(ifd0=None, exif=None, gps=None, big_endian=False, tail=b""):
    """'Exif\\0\\0' + a TIFF structure written by Pillow, `tail` appended (a thumbnail's place)"""
    ex = Image.Exif()
    ex.endian = ">" if big_endian else "<"
    for k, v in (ifd0 or {}).items():
        ex[k] = v
    if exif:
        ex.get_ifd(0x8769).update(exif)
    if gps:
        ex.get_ifd(0x8825).update(gps)
    data = ex.tobytes()
    if data[:6] != b"Exif\0\0":
        data = b"Exif\0\0" + data
    assert data[:6] == b"Exif\0\0" and data[6:8] == (b"MM" if big_endian else b"II")
    return data + tail


def xmp_packet(values, elements=False, about="", extra_attributes=""):
    ns = ('xmlns:rdf="http://www.w3.org/1999/02/22-rdf-syntax-ns#" xmlns:tiff="http://ns.adobe.com/tiff/1.0/" '
          'xmlns:drone-dji="http://www.dji.com/drone-dji/1.0/" xmlns:Camera="http://pix4d.com/camera/1.0/"')
    if elements:
        body = "".join(f"\n   <{k}>{v}</{k}>" for k, v in values.items())
        desc = f'<rdf:Description rdf:about="{about}" {ns}{extra_attributes}>{body}\n  </rdf:Description>'
    else:
        attrs = "".join(f'\n    {k}="{v}"' for k, v in values.items())
        desc = f'<rdf:Description rdf:about="{about}" {ns}{extra_attributes}{attrs}/>'
    text = ('<?xpacket begin="﻿" id="W5M0MpCehiHzreSzNTczkc9d"?>\n<x:xmpmeta xmlns:x="adobe:ns:meta/">\n <rdf:RDF '
            'xmlns:rdf="http://www.w3.org/1999/02/22-rdf-syntax-ns#">\n  ' + desc + '\n </rdf:RDF>\n</x:xmpmeta>\n<?xpacket end="w"?>')
    return XMP_ID + text.encode("utf-8")


def dms(value):
    """degrees as three rationals: degrees, minutes, seconds / 10000"""
    value = abs(value)
    d = int(value)
    m = int((value - d) * 60)
    s = round(((value - d) * 60 - m) * 60 * 10000)
    return (R(d, 1), R(m, 1), R(s, 10000))


def gps_ifd(lat, lon, alt=None, alt_ref=0, date=None, time=None, datum=None):
    g = {1: "N" if lat >= 0 else "S", 2: dms(lat), 3: "E" if lon >= 0 else "W", 4: dms(lon)}
    if alt is not None:
        g[5] = bytes([alt_ref])
        g[6] = alt
    if time is not None:
        g[7] = time
    if datum is not None:
        g[18] = datum
    if date is not None:
        g[29] = date
    return g


DJI = {"drone-dji:AbsoluteAltitude": "+512.35", "drone-dji:RelativeAltitude": "+80.10", "drone-dji:GimbalRollDegree": "+0.00",
       "drone-dji:GimbalYawDegree": "-112.40", "drone-dji:GimbalPitchDegree": "-89.90",
       "drone-dji:CalibratedFocalLength": "3666.666504", "drone-dji:CalibratedOpticalCenterX": "2736.000000",
       "drone-dji:CalibratedOpticalCenterY": "1824.000000"}


def cases():
    """name -> the file's bytes"""
    size = {0xa002: W, 0xa003: H}
    thumb = splice(base_jpeg(16, 12, seed=9), [exif_bytes({0x010f: "THUMB", 0x0110: "inner"}, {0xa405: 99},
                                                          gps_ifd(1.5, 2.5, R(7, 1)))])
    out = {}
    out["le_north_east_35mm"] = splice(base_jpeg(seed=1), [exif_bytes(
        {0x010f: "Acme", 0x0110: "Surveyor 2", 0x0132: "2024:05:01 10:00:00"},
        {**size, 0x9003: "2024:05:01 10:00:01", 0x9291: "37", 0xa405: 24, 0xa431: "SN-0042", 0xa433: "Acme Optics",
         0xa434: "AO 8.8mm f/2.8"}, gps_ifd(47.376912, 8.541694, R(4321, 10), 0))])
    out["be_south_west_cm"] = splice(base_jpeg(seed=2), [exif_bytes(
        {0x010f: "Acme", 0x0110: "Surveyor 2", 0x0132: "2024:05:01 11:00:00"},
        {**size, 0x920a: R(88, 10), 0xa20e: R(12500, 3), 0xa210: 3},
        gps_ifd(-33.9, -151.234567, R(125, 10), 1, date="2024:05:01", time=(R(11, 1), R(0, 1), R(1234, 100)), datum="WGS-84"),
        big_endian=True)])
    out["le_inch"] = splice(base_jpeg(seed=3), [exif_bytes(
        {0x010f: "Acme", 0x0110: "Inch"}, {**size, 0x920a: R(50, 10), 0xa20e: R(10583, 1), 0xa210: 2}, gps_ifd(0.25, -0.5, R(10, 1)))])
    out["dji_attributes"] = splice(base_jpeg(seed=4), [
        exif_bytes({0x010f: "DJI", 0x0110: "FC6310"}, dict(size), gps_ifd(47.3771, 8.5421, R(5120, 10))), xmp_packet(DJI)])
    out["dji_elements"] = splice(base_jpeg(seed=5), [
        exif_bytes({0x0110: "unnamed"}, dict(size), gps_ifd(47.3772, 8.5422, R(5121, 10)), big_endian=True),
        xmp_packet(DJI, elements=True, about="DJI Meta Data")])
    out["camera_packet"] = splice(base_jpeg(seed=6), [
        exif_bytes({0x010f: "senseFly", 0x0110: "S.O.D.A."}, {**size, 0xa405: 29}, gps_ifd(46.5, 6.6, R(600, 1))),
        xmp_packet({"Camera:Roll": "1.5", "Camera:Pitch": "3.25", "Camera:Yaw": "271", "Camera:GPSXYAccuracy": "0.02",
                    "Camera:GPSZAccuracy": "3/100"})])
    out["xmp_before_exif"] = splice(base_jpeg(seed=7), [
        xmp_packet({**DJI, "tiff:ImageWidth": str(W), "tiff:ImageLength": str(H)}, about="DJI Meta Data"),
        exif_bytes({0x010f: "DJI", 0x0110: "FC6310"}, None, gps_ifd(47.3773, 8.5423, R(5122, 10)))])
    out["thumbnail_in_app1"] = splice(base_jpeg(seed=8), [
        exif_bytes({0x010f: "DJI", 0x0110: "FC6310"}, {**size, 0xa405: 24}, gps_ifd(47.3774, 8.5424, R(5123, 10)), tail=thumb),
        xmp_packet({k: v for k, v in DJI.items() if "Calibrated" not in k})])
    out["no_app1"] = base_jpeg(seed=9)
    out["zero_denominator"] = splice(base_jpeg(seed=10), [exif_bytes(
        {0x010f: "Acme", 0x0110: "Zero"}, {**size, 0x920a: R(88, 10), 0xa20e: R(5, 0), 0xa405: 24}, gps_ifd(10.0, 20.0, R(5, 0)))])
    return out


# ---- Pillow's reading, mapped as extract_metadata maps its reader's fields ---------------------------------------------
def _rational(v):
    """a Pillow rational (or number) as a float; None where the denominator is 0"""
    if v is None:
        return None
    if getattr(v, "denominator", 1) == 0:
        return None
    return float(v)


def _text(v):
    if v is None:
        return None
    if isinstance(v, bytes):
        v = v.decode("latin-1")
    return str(v).split("\0")[0].rstrip(" ")


def _xmp_value(xmp, name):
    m = re.search(r'[\s]' + re.escape(name) + r'\s*=\s*"([^"]*)"', xmp) or re.search(r"<" + re.escape(name) + r">([^<]+)</", xmp)
    if not m:
        return None
    parts = m.group(1).split("/")

    def num(s):
        m2 = re.match(r"\s*[+-]?(\d+\.?\d*([eE][+-]?\d+)?|\.\d+([eE][+-]?\d+)?)", s)
        return float(m2.group(0)) if m2 else 0.0
    return num(parts[0]) if len(parts) == 1 else num(parts[0]) / num(parts[1]) if len(parts) == 2 else None


def _degrees(triple, ref, negative):
    if triple is None or len(triple) != 3:
        return None
    d, m, s = (_rational(v) for v in triple)
    if d is None:
        return None
    value = d + (m or 0.0) / 60 + (s or 0.0) / 3600
    if isinstance(ref, bytes):
        ref = ref.decode("latin-1")
    return -value if ref and ref[0] == negative else value


def pillow_metadata(data):
    """(metadata dict in graph.json's layout, status) from Pillow's getexif(), get_ifd() and info["xmp"]"""
    nan = math.nan
    camera = dict(dimensions=[0, 0], focal_length_px=nan, principal=[nan, nan], make="", model="", serial_no="", lens_make="",
                  lens_model="")
    capture = dict(latitude=nan, longitude=nan, altitude=nan, relative_altitude=nan, roll=nan, pitch=nan, yaw=nan,
                   accuracy_xy=nan, accuracy_z=nan, datum="", timestamp="", datestamp="")
    out = dict(camera_info=camera, capture_info=capture)
    im = Image.open(io.BytesIO(data))
    has_exif = "exif" in im.info
    xmp = im.info.get("xmp")
    if not has_exif and xmp is None:
        return out, "absent"
    ifd0 = im.getexif() if has_exif else {}
    sub = ifd0.get_ifd(0x8769) if has_exif else {}
    gps = ifd0.get_ifd(0x8825) if has_exif else {}
    both = {**dict(ifd0), **dict(sub)}  # IFD0 is read for Exif tags too; the Exif IFD's come later and win
    xmp = xmp.decode("utf-8", "replace") if isinstance(xmp, bytes) else xmp
    xmp_first = xmp is not None and has_exif and data.find(XMP_ID) < data.find(b"Exif\0\0")
    make = _text(ifd0.get(0x010f)) or ""

    width, height = both.get(0xa002, 0), both.get(0xa003, 0)
    altitude = _rational(gps.get(6))
    if altitude is not None:
        ref = gps.get(5, 0)
        ref = ref[0] if isinstance(ref, (bytes, tuple)) else ref
        altitude = -altitude if ref == 1 else altitude
    relative = roll = pitch = yaw = None
    calibrated = cx = cy = 0.0
    acc_xy = acc_z = 0.0
    if xmp is not None:
        if xmp_first or (width == 0 and height == 0):  # the packet's size counts only while EXIF has given none
            w2, h2 = _xmp_value(xmp, "tiff:ImageWidth"), _xmp_value(xmp, "tiff:ImageHeight")
            h2 = h2 if h2 is not None else _xmp_value(xmp, "tiff:ImageLength")
            # read before the Exif segment, the Exif size tags replace it where they exist
            width, height = width or int(w2 or 0), height or int(h2 or 0)
        make_then = "" if xmp_first else make
        about = re.search(r'rdf:about\s*=\s*"([^"]*)"', xmp)
        if make_then.lower() == "dji" or (about and about.group(1).lower() == "dji meta data"):
            v = _xmp_value(xmp, "drone-dji:AbsoluteAltitude")
            if v is not None and not (xmp_first and altitude is not None):
                altitude = v
            relative = _xmp_value(xmp, "drone-dji:RelativeAltitude")
            roll, pitch, yaw = (_xmp_value(xmp, f"drone-dji:Gimbal{k}Degree") for k in ("Roll", "Pitch", "Yaw"))
            calibrated = _xmp_value(xmp, "drone-dji:CalibratedFocalLength") or 0.0
            cx = _xmp_value(xmp, "drone-dji:CalibratedOpticalCenterX") or 0.0
            cy = _xmp_value(xmp, "drone-dji:CalibratedOpticalCenterY") or 0.0
        elif make_then.lower() in ("sensefly", "sentera"):
            roll, pitch, yaw = (_xmp_value(xmp, f"Camera:{k}") for k in ("Roll", "Pitch", "Yaw"))
            if pitch is not None:
                d = math.fmod(pitch - 90.0 + 180.0, 360.0)
                pitch = d + 180.0 if d < 0 else d - 180.0
            acc_xy = _xmp_value(xmp, "Camera:GPSXYAccuracy") or 0.0
            acc_z = _xmp_value(xmp, "Camera:GPSZAccuracy") or 0.0

    original = _text(both.get(0x9003)) or ""
    capture["timestamp"] = original + (_text(both.get(0x9291)) or "") if original else (_text(ifd0.get(0x0132)) or "")
    lat = _degrees(gps.get(2), gps.get(1), "S")
    lon = _degrees(gps.get(4), gps.get(3), "W")
    if lat is not None and lon is not None:
        capture["latitude"], capture["longitude"] = lat, lon
        if acc_xy > 0:
            capture["accuracy_xy"] = acc_xy
        capture["datum"] = _text(gps.get(18)) or ""
        if _text(gps.get(29)):
            t = gps.get(7)
            stamp = "%g %g %g" % tuple(_rational(v) or 0.0 for v in t) if t is not None and len(t) == 3 else ""
            capture["timestamp"] = _text(gps.get(29)) + " " + stamp
    if altitude is not None:
        capture["altitude"] = altitude
        if acc_z > 0:
            capture["accuracy_z"] = acc_z
    if relative is not None:
        capture["altitude"], capture["accuracy_z"] = relative, acc_z
    if roll is not None and pitch is not None and yaw is not None:
        capture["roll"], capture["pitch"], capture["yaw"] = roll, pitch, yaw

    camera["dimensions"] = [int(width), int(height)]
    camera["make"], camera["model"] = make, _text(ifd0.get(0x0110)) or ""
    camera["serial_no"] = _text(both.get(0xa431)) or ""
    camera["lens_make"], camera["lens_model"] = _text(both.get(0xa433)) or "", _text(both.get(0xa434)) or ""
    f35 = _rational(both.get(0xa405)) or 0.0
    focal, xres = _rational(both.get(0x920a)) or 0.0, _rational(both.get(0xa20e)) or 0.0
    if calibrated > 1:
        camera["focal_length_px"] = calibrated
    elif f35 > 0:
        camera["focal_length_px"] = f35 / 43.27 * math.hypot(width, height)
    elif focal > 0 and xres > 0:
        camera["focal_length_px"] = focal / ((10 if both.get(0xa210) == 3 else 25.4) / xres)
    if cx > 0 and cy > 0:
        camera["principal"] = [cy, cx]
    return out, "ok"


def main():
    here = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "survey_files")
    os.makedirs(here, exist_ok=True)
    expected = {}
    for name, data in cases().items():
        with open(os.path.join(here, name + ".jpg"), "wb") as f:
            f.write(data)
        md, status = pillow_metadata(data)
        expected[name] = dict(status=status, metadata=md)
    with open(os.path.join(here, "expected.json"), "w") as f:
        json.dump(expected, f, indent=1)
        f.write("\n")
    print(f"{len(expected)} files in {here}")


if __name__ == "__main__":
    main()
