#include "image_metadata.hpp"

#include <algorithm>
#include <cfloat>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <strings.h>

namespace opencalibration_amd
{
namespace
{

// ---- the reader's fields (TinyEXIF.h's EXIFInfo, the ones extract_metadata reads), with its "not there" values ----------
struct Fields
{
    bool exif = false, xmp = false;
    std::string Make, Model, SerialNumber, DateTime, DateTimeOriginal, SubSecTimeOriginal, LensMake, LensModel;
    uint32_t ImageWidth = 0, ImageHeight = 0;
    double FocalLength = 0, FocalLengthIn35mm = 0, FocalPlaneXResolution = 0;
    uint16_t FocalPlaneResolutionUnit = 0;
    double CalibFocalLength = 0, OpticalCenterX = 0, OpticalCenterY = 0;
    double Latitude = DBL_MAX, Longitude = DBL_MAX, Altitude = DBL_MAX, RelativeAltitude = DBL_MAX;
    double RollDegree = DBL_MAX, PitchDegree = DBL_MAX, YawDegree = DBL_MAX;
    double AccuracyXY = 0, AccuracyZ = 0;
    uint8_t AltitudeRef = 0;
    std::string GPSMapDatum, GPSTimeStamp, GPSDateStamp;
    struct Coord
    {
        double degrees = DBL_MAX, minutes = 0, seconds = 0;
        uint8_t direction = 0;
    } Lat, Lon;
};

// ---- TIFF structure: every read is inside [t, t + n) ----------------------------------------------------------------
struct Tiff
{
    const uint8_t *t;
    size_t n;
    bool intel;
    bool has(uint64_t off, uint64_t bytes) const
    {
        return off <= n && bytes <= n - off;
    }
    uint16_t u16(size_t off) const
    {
        return intel ? (uint16_t)(t[off] | (t[off + 1] << 8)) : (uint16_t)((t[off] << 8) | t[off + 1]);
    }
    uint32_t u32(size_t off) const
    {
        return intel ? ((uint32_t)t[off + 3] << 24) | ((uint32_t)t[off + 2] << 16) | ((uint32_t)t[off + 1] << 8) | t[off]
                     : ((uint32_t)t[off] << 24) | ((uint32_t)t[off + 1] << 16) | ((uint32_t)t[off + 2] << 8) | t[off + 3];
    }
};

struct Entry // one 12-byte directory entry at `at`, which its IFD's bound check has placed inside the segment
{
    const Tiff &tf;
    size_t at;
    uint16_t tag, format;
    uint32_t count;
    Entry(const Tiff &tiff, size_t where) : tf(tiff), at(where), tag(tiff.u16(where)), format(tiff.u16(where + 2)), count(tiff.u32(where + 4))
    {
    }
    uint32_t data() const
    {
        return tf.u32(at + 8);
    }
    bool fetch(std::string &v) const // ASCII; up to four bytes sit in the entry, more at the offset
    {
        if (format != 2 || count == 0)
            return false;
        if (count <= 4)
        {
            v.assign((const char *)tf.t + at + 8, count);
            if (v.back() == '\0')
                v.pop_back();
            return true;
        }
        v.clear();
        if (tf.has(data(), count))
        {
            const char *s = (const char *)tf.t + data();
            size_t k = 0;
            while (k < count && s[k] != '\0')
                k++;
            while (k && s[k - 1] == ' ')
                k--;
            v.assign(s, k);
        }
        return true;
    }
    bool fetch(uint8_t &v) const
    {
        if ((format != 1 && format != 2 && format != 6) || count == 0)
            return false;
        v = tf.t[at + 8];
        return true;
    }
    bool fetch(uint16_t &v) const
    {
        if (format != 3 || count == 0)
            return false;
        v = tf.u16(at + 8);
        return true;
    }
    bool fetch(uint32_t &v) const
    {
        if (format != 4 || count == 0)
            return false;
        v = tf.u32(at + 8);
        return true;
    }
    bool fetch(double &v, uint32_t idx = 0) const // (S)RATIONAL; a zero denominator or a place outside the segment: not there
    {
        if ((format != 5 && format != 10) || count <= idx)
            return false;
        const uint64_t off = (uint64_t)data() + 8ull * idx;
        if (!tf.has(off, 8))
            return false;
        const uint32_t num = tf.u32((size_t)off), den = tf.u32((size_t)off + 4);
        if (den == 0)
            return false;
        v = format == 10 ? (double)(int32_t)num / (double)(int32_t)den : (double)num / (double)den;
        return true;
    }
    bool fetch_long_or_short(uint32_t &v) const
    {
        uint16_t s;
        if (fetch(v))
            return true;
        if (!fetch(s))
            return false;
        v = s;
        return true;
    }
};

// ---- XMP: the first rdf:Description of the packet, its attributes and its child elements ------------------------------
size_t find(const char *b, size_t from, size_t to, const char *needle)
{
    const size_t k = std::strlen(needle);
    if (from > to || to - from < k)
        return std::string::npos;
    const char *hit = std::search(b + from, b + to, needle, needle + k);
    return hit == b + to ? std::string::npos : (size_t)(hit - b);
}

bool is_space(char c)
{
    return c == ' ' || c == '\t' || c == '\r' || c == '\n';
}

struct Xmp
{
    const char *b = nullptr;
    size_t attr_from = 0, tag_end = 0, desc_end = 0; // the start tag's attributes, its '>', the element's end

    bool locate(const char *text, size_t len)
    {
        b = text;
        const size_t tail = find(b, 0, len, "<?xpacket end=");
        if (tail != std::string::npos)
            len = tail;
        size_t d = 0;
        for (;;)
        {
            d = find(b, d, len, "<rdf:Description");
            if (d == std::string::npos)
                return false;
            d += 16;
            if (d < len && (is_space(b[d]) || b[d] == '>' || b[d] == '/'))
                break;
        }
        attr_from = d;
        char quote = 0;
        size_t i = d;
        for (; i < len; i++)
        {
            if (quote)
                quote = b[i] == quote ? 0 : quote;
            else if (b[i] == '"' || b[i] == '\'')
                quote = b[i];
            else if (b[i] == '>')
                break;
        }
        if (i >= len)
            return false;
        tag_end = i;
        if (b[i - 1] == '/')
            desc_end = i; // self-closed: no children
        else
        {
            const size_t close = find(b, i, len, "</rdf:Description>");
            desc_end = close == std::string::npos ? len : close;
        }
        return true;
    }
    bool attribute(const char *name, std::string &v) const
    {
        const size_t k = std::strlen(name);
        size_t i = attr_from;
        while (i < tag_end)
        {
            while (i < tag_end && (is_space(b[i]) || b[i] == '/'))
                i++;
            const size_t n0 = i;
            while (i < tag_end && !is_space(b[i]) && b[i] != '=')
                i++;
            const size_t n1 = i;
            while (i < tag_end && is_space(b[i]))
                i++;
            if (i >= tag_end || b[i] != '=')
                return false;
            i++;
            while (i < tag_end && is_space(b[i]))
                i++;
            if (i >= tag_end || (b[i] != '"' && b[i] != '\''))
                return false;
            const char quote = b[i++];
            const size_t v0 = i;
            while (i < tag_end && b[i] != quote)
                i++;
            if (i >= tag_end)
                return false;
            if (n1 - n0 == k && !std::memcmp(b + n0, name, k))
            {
                v.assign(b + v0, i - v0);
                return true;
            }
            i++;
        }
        return false;
    }
    bool element(const char *name, std::string &v) const
    {
        const std::string open = std::string("<") + name;
        size_t i = tag_end;
        while ((i = find(b, i, desc_end, open.c_str())) != std::string::npos)
        {
            i += open.size();
            if (i >= desc_end || !(is_space(b[i]) || b[i] == '>' || b[i] == '/'))
                continue;
            while (i < desc_end && b[i] != '>')
                i++;
            if (i >= desc_end || b[i - 1] == '/')
                return false;
            const size_t v0 = ++i;
            while (i < desc_end && b[i] != '<')
                i++;
            if (i == v0)
                return false;
            v.assign(b + v0, i - v0);
            return true;
        }
        return false;
    }
    bool text(const char *name, std::string &v) const
    {
        return attribute(name, v) || element(name, v);
    }
    bool value(const char *name, double &out) const // a number or a fraction "a/b", by strtod
    {
        std::string s;
        if (!text(name, s))
            return false;
        const size_t slash = s.find('/');
        if (slash == std::string::npos)
        {
            out = std::strtod(s.c_str(), nullptr);
            return true;
        }
        if (s.find('/', slash + 1) != std::string::npos)
            return false;
        out = std::strtod(s.substr(0, slash).c_str(), nullptr) / std::strtod(s.c_str() + slash + 1, nullptr);
        return true;
    }
    bool value(const char *name, uint32_t &out) const
    {
        std::string s;
        if (!text(name, s))
            return false;
        char *end = nullptr;
        const unsigned long v = std::strtoul(s.c_str(), &end, 10);
        if (end == s.c_str())
            return false;
        out = (uint32_t)v;
        return true;
    }
};

double norm_d180(double d)
{
    return (d = std::fmod(d + 180.0, 360.0)) < 0 ? d + 180.0 : d - 180.0;
}

bool make_is(const Fields &f, const char *name)
{
    return 0 == strcasecmp(f.Make.c_str(), name);
}

// parseFromXMPSegmentXML (TinyEXIF.cpp:1038-1162): false = no rdf:Description to read, the segment counts as absent
bool parse_xmp(const char *text, size_t len, Fields &f)
{
    Xmp x;
    if (!x.locate(text, len))
        return false;
    if (f.ImageWidth == 0 && f.ImageHeight == 0)
    {
        x.value("tiff:ImageWidth", f.ImageWidth);
        if (!x.value("tiff:ImageHeight", f.ImageHeight))
            x.value("tiff:ImageLength", f.ImageHeight);
    }
    std::string about;
    const bool dji_about = x.attribute("rdf:about", about) && 0 == strcasecmp(about.c_str(), "DJI Meta Data");
    if (make_is(f, "DJI") || dji_about)
    {
        x.value("drone-dji:AbsoluteAltitude", f.Altitude);
        x.value("drone-dji:RelativeAltitude", f.RelativeAltitude);
        x.value("drone-dji:GimbalRollDegree", f.RollDegree);
        x.value("drone-dji:GimbalPitchDegree", f.PitchDegree);
        x.value("drone-dji:GimbalYawDegree", f.YawDegree);
        x.value("drone-dji:CalibratedFocalLength", f.CalibFocalLength);
        x.value("drone-dji:CalibratedOpticalCenterX", f.OpticalCenterX);
        x.value("drone-dji:CalibratedOpticalCenterY", f.OpticalCenterY);
    }
    else if (make_is(f, "senseFly") || make_is(f, "Sentera"))
    {
        x.value("Camera:Roll", f.RollDegree);
        if (x.value("Camera:Pitch", f.PitchDegree))
            f.PitchDegree = norm_d180(f.PitchDegree - 90.0); // pitch 0 is nadir there, -90 in the DJI convention
        x.value("Camera:Yaw", f.YawDegree);
        x.value("Camera:GPSXYAccuracy", f.AccuracyXY);
        x.value("Camera:GPSZAccuracy", f.AccuracyZ);
    }
    else if (make_is(f, "PARROT"))
    {
        x.value("Camera:Roll", f.RollDegree) || x.value("drone-parrot:CameraRollDegree", f.RollDegree);
        if (x.value("Camera:Pitch", f.PitchDegree) || x.value("drone-parrot:CameraPitchDegree", f.PitchDegree))
            f.PitchDegree = norm_d180(f.PitchDegree - 90.0);
        x.value("Camera:Yaw", f.YawDegree) || x.value("drone-parrot:CameraYawDegree", f.YawDegree);
        x.value("Camera:AboveGroundAltitude", f.RelativeAltitude);
    }
    return true;
}

// ---- the three directories (TinyEXIF.cpp:351-761) -------------------------------------------------------------------
void exif_tag(const Entry &e, Fields &f)
{
    switch (e.tag)
    {
    case 0x02bc: // the XMP packet as a TIFF tag
        if (e.format == 7 && e.count > 4 && e.tf.has(e.data(), e.count))
        {
            const char *s = (const char *)e.tf.t + e.data();
            parse_xmp(s, strnlen(s, e.count), f);
        }
        break;
    case 0x9003:
        e.fetch(f.DateTimeOriginal);
        break;
    case 0x920a:
        e.fetch(f.FocalLength);
        break;
    case 0x9291:
        e.fetch(f.SubSecTimeOriginal);
        break;
    case 0xa002:
        e.fetch_long_or_short(f.ImageWidth);
        break;
    case 0xa003:
        e.fetch_long_or_short(f.ImageHeight);
        break;
    case 0xa20e:
        e.fetch(f.FocalPlaneXResolution);
        break;
    case 0xa210:
        e.fetch(f.FocalPlaneResolutionUnit);
        break;
    case 0xa405:
        if (!e.fetch(f.FocalLengthIn35mm))
        {
            uint16_t s;
            if (e.fetch(s))
                f.FocalLengthIn35mm = (double)s;
        }
        break;
    case 0xa431:
        e.fetch(f.SerialNumber);
        break;
    case 0xa433:
        e.fetch(f.LensMake);
        break;
    case 0xa434:
        e.fetch(f.LensModel);
        break;
    }
}

void image_tag(const Entry &e, Fields &f, uint64_t &exif_ifd, uint64_t &gps_ifd)
{
    switch (e.tag)
    {
    case 0x010f:
        e.fetch(f.Make);
        break;
    case 0x0110:
        e.fetch(f.Model);
        break;
    case 0x0132:
        e.fetch(f.DateTime);
        break;
    case 0x8769:
        exif_ifd = e.data();
        break;
    case 0x8825:
        gps_ifd = e.data();
        break;
    default:
        exif_tag(e, f); // some files keep Exif tags in IFD0
        break;
    }
}

void gps_tag(const Entry &e, Fields &f)
{
    switch (e.tag)
    {
    case 1:
        e.fetch(f.Lat.direction);
        break;
    case 2:
        if ((e.format == 5 || e.format == 10) && e.count == 3)
        {
            e.fetch(f.Lat.degrees, 0);
            e.fetch(f.Lat.minutes, 1);
            e.fetch(f.Lat.seconds, 2);
        }
        break;
    case 3:
        e.fetch(f.Lon.direction);
        break;
    case 4:
        if ((e.format == 5 || e.format == 10) && e.count == 3)
        {
            e.fetch(f.Lon.degrees, 0);
            e.fetch(f.Lon.minutes, 1);
            e.fetch(f.Lon.seconds, 2);
        }
        break;
    case 5:
        e.fetch(f.AltitudeRef);
        break;
    case 6:
        e.fetch(f.Altitude);
        break;
    case 7:
        if ((e.format == 5 || e.format == 10) && e.count == 3)
        {
            double h = 0, m = 0, s = 0;
            e.fetch(h, 0);
            e.fetch(m, 1);
            e.fetch(s, 2);
            char buffer[256];
            std::snprintf(buffer, sizeof buffer, "%g %g %g", h, m, s);
            f.GPSTimeStamp = buffer;
        }
        break;
    case 18:
        e.fetch(f.GPSMapDatum);
        break;
    case 29:
        e.fetch(f.GPSDateStamp);
        break;
    }
}

void parse_coords(Fields &f) // Geolocation_t::parseCoords (TinyEXIF.cpp:1166-1194)
{
    if (f.Lat.degrees != DBL_MAX || f.Lat.minutes != 0 || f.Lat.seconds != 0)
    {
        f.Latitude = f.Lat.degrees + f.Lat.minutes / 60 + f.Lat.seconds / 3600;
        if ('S' == f.Lat.direction)
            f.Latitude = -f.Latitude;
    }
    if (f.Lon.degrees != DBL_MAX || f.Lon.minutes != 0 || f.Lon.seconds != 0)
    {
        f.Longitude = f.Lon.degrees + f.Lon.minutes / 60 + f.Lon.seconds / 3600;
        if ('W' == f.Lon.direction)
            f.Longitude = -f.Longitude;
    }
    if (f.Altitude != DBL_MAX && f.AltitudeRef == 1)
        f.Altitude = -f.Altitude;
}

enum Segment
{
    SEG_OK,
    SEG_ABSENT,
    SEG_CORRUPT
};

// the number of a directory's entries, or -1 where the directory (count, entries, next-IFD link) leaves the segment
int directory(const Tiff &tf, uint64_t off)
{
    if (!tf.has(off, 2))
        return -1;
    const int num = tf.u16((size_t)off);
    return tf.has(off, 6 + 12ull * (unsigned)num) ? num : -1;
}

// parseFromEXIFSegment (TinyEXIF.cpp:926-1015) over an APP1 payload
Segment parse_exif(const uint8_t *p, size_t len, Fields &f)
{
    if (len < 6 || std::memcmp(p, "Exif\0\0", 6) != 0)
        return SEG_ABSENT;
    if (len < 14)
        return SEG_CORRUPT;
    Tiff tf{p + 6, len - 6, false};
    if (tf.t[0] == 'I' && tf.t[1] == 'I')
        tf.intel = true;
    else if (tf.t[0] != 'M' || tf.t[1] != 'M')
        return SEG_CORRUPT;
    if (tf.u16(2) != 0x2a)
        return SEG_CORRUPT;
    const uint64_t ifd0 = tf.u32(4);
    int num = directory(tf, ifd0);
    if (ifd0 < 8 || num < 0)
        return SEG_CORRUPT;
    uint64_t exif_ifd = tf.n, gps_ifd = tf.n; // "none": the test below fails for them
    for (int i = 0; i < num; i++)
        image_tag(Entry(tf, (size_t)ifd0 + 2 + 12 * (size_t)i), f, exif_ifd, gps_ifd);
    if (tf.has(exif_ifd, 4))
    {
        if ((num = directory(tf, exif_ifd)) < 0)
            return SEG_CORRUPT;
        for (int i = 0; i < num; i++)
            exif_tag(Entry(tf, (size_t)exif_ifd + 2 + 12 * (size_t)i), f);
    }
    if (tf.has(gps_ifd, 4))
    {
        if ((num = directory(tf, gps_ifd)) < 0)
            return SEG_CORRUPT;
        for (int i = 0; i < num; i++)
            gps_tag(Entry(tf, (size_t)gps_ifd + 2 + 12 * (size_t)i), f);
        parse_coords(f);
    }
    return SEG_OK;
}

const char XMP_ID[] = "http://ns.adobe.com/xap/1.0/"; // with its NUL: 29 bytes

Segment parse_xmp_segment(const uint8_t *p, size_t len, Fields &f)
{
    if (len < sizeof XMP_ID || std::memcmp(p, XMP_ID, sizeof XMP_ID) != 0)
        return SEG_ABSENT;
    return parse_xmp((const char *)p + sizeof XMP_ID, len - sizeof XMP_ID, f) ? SEG_OK : SEG_ABSENT;
}

// EXIFInfo::parseFrom (TinyEXIF.cpp:768-853): the markers up to SOS, APP1 by its length - the thumbnail JPEG a camera
// file carries inside APP1 is never walked
MetadataStatus read_fields(const uint8_t *d, size_t n, Fields &f)
{
    const auto done = [&](MetadataStatus otherwise) { return f.exif || f.xmp ? METADATA_OK : otherwise; };
    if (n < 2 || d[0] != 0xFF || d[1] != 0xD8)
        return METADATA_CORRUPT;
    size_t at = 2;
    for (;;)
    {
        if (at + 2 > n)
            return done(METADATA_CORRUPT); // the file ends before SOS
        if (d[at] != 0xFF)
            return done(METADATA_CORRUPT);
        while (at < n && d[at] == 0xFF) // fill bytes
            at++;
        if (at >= n)
            return done(METADATA_CORRUPT);
        const int m = d[at++];
        if (m == 0x00 || m == 0x01 || m == 0xD8 || (m >= 0xD0 && m <= 0xD7))
            continue;
        if (m == 0xDA || m == 0xD9)
            return done(METADATA_ABSENT);
        if (at + 2 > n)
            return done(METADATA_CORRUPT);
        const size_t seg = ((size_t)d[at] << 8) | d[at + 1];
        if (seg < 2 || seg > n - at)
            return done(METADATA_CORRUPT);
        if (m == 0xE1 && seg > 2)
        {
            const uint8_t *p = d + at + 2;
            const size_t len = seg - 2;
            Segment s = parse_exif(p, len, f);
            if (s == SEG_OK)
                f.exif = true;
            else if (s == SEG_ABSENT)
            {
                s = parse_xmp_segment(p, len, f);
                if (s == SEG_OK)
                    f.xmp = true;
            }
            if (s == SEG_CORRUPT)
                return done(METADATA_CORRUPT);
            if (f.exif && f.xmp)
                return METADATA_OK;
        }
        at += seg;
    }
}

} // namespace

MetadataStatus extract_metadata(const uint8_t *data, size_t size, image_metadata &res)
{
    res = image_metadata();
    Fields f;
    const MetadataStatus status = data ? read_fields(data, size, f) : METADATA_CORRUPT;
    if (status != METADATA_OK)
        return status;

    // extract_metadata.cpp:60-145
    auto &cap = res.capture_info;
    auto &cam = res.camera_info;
    cap.timestamp = f.DateTimeOriginal.size() > 0 ? f.DateTimeOriginal + f.SubSecTimeOriginal : f.DateTime;
    if (f.Latitude != DBL_MAX && f.Longitude != DBL_MAX)
    {
        cap.latitude = f.Latitude;
        cap.longitude = f.Longitude;
        if (f.AccuracyXY > 0)
            cap.accuracyXY = f.AccuracyXY;
        cap.datum = f.GPSMapDatum;
        if (f.GPSDateStamp.size() > 0)
            cap.timestamp = f.GPSDateStamp + " " + f.GPSTimeStamp;
    }
    if (f.Altitude != DBL_MAX)
    {
        cap.altitude = f.Altitude;
        if (f.AccuracyZ > 0)
            cap.accuracyZ = f.AccuracyZ;
    }
    if (f.RelativeAltitude != DBL_MAX) // the height above the take-off point replaces the altitude
    {
        cap.altitude = f.RelativeAltitude;
        cap.accuracyZ = f.AccuracyZ;
    }
    if (f.RollDegree != DBL_MAX && f.PitchDegree != DBL_MAX && f.YawDegree != DBL_MAX)
    {
        cap.rollDegree = f.RollDegree;
        cap.pitchDegree = f.PitchDegree;
        cap.yawDegree = f.YawDegree;
    }
    cam.width_px = f.ImageWidth;
    cam.height_px = f.ImageHeight;
    cam.make = f.Make;
    cam.model = f.Model;
    cam.serial_no = f.SerialNumber;
    cam.lens_make = f.LensMake;
    cam.lens_model = f.LensModel;
    if (f.CalibFocalLength > 1)
        cam.focal_length_px = f.CalibFocalLength;
    else if (f.FocalLengthIn35mm > 0)
        cam.focal_length_px = f.FocalLengthIn35mm / 43.27 * std::hypot((double)cam.width_px, (double)cam.height_px);
    else if (f.FocalLength > 0 && f.FocalPlaneXResolution > 0)
    {
        const double scale = f.FocalPlaneResolutionUnit == 3 ? 10 : 25.4; // centimetres, else inches
        const double pixel_size_mm = scale / f.FocalPlaneXResolution;
        cam.focal_length_px = f.FocalLength / pixel_size_mm;
    }
    if (f.OpticalCenterX > 0 && f.OpticalCenterY > 0)
    {
        cam.principal_point_px[0] = f.OpticalCenterY; // swapped, as extract_metadata.cpp:141-145 has them
        cam.principal_point_px[1] = f.OpticalCenterX;
    }
    return status;
}

} // namespace opencalibration_amd
