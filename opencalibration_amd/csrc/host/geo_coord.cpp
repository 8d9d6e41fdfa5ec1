#include "geo_coord.hpp"

#include <cmath>
#include <complex>
#include <cstdio>
#include <cstdlib>

namespace opencalibration_amd
{
namespace
{

constexpr double WGS84_A = 6378137.0, WGS84_F = 1.0 / 298.257223563;
constexpr double DEG = 0.017453292519943295769236907684886;

struct Series
{
    double e, e2m, A, alp[7], bet[7];
    Series()
    {
        const double n = WGS84_F / (2 - WGS84_F), n2 = n * n, n3 = n2 * n, n4 = n2 * n2, n5 = n4 * n, n6 = n3 * n3;
        e = std::sqrt(WGS84_F * (2 - WGS84_F));
        e2m = (1 - WGS84_F) * (1 - WGS84_F);
        A = WGS84_A / (1 + n) * (1 + n2 / 4 + n4 / 64 + n6 / 256);
        alp[0] = bet[0] = 0;
        // Karney 2011 eq. 35
        alp[1] = n / 2 - 2 * n2 / 3 + 5 * n3 / 16 + 41 * n4 / 180 - 127 * n5 / 288 + 7891 * n6 / 37800;
        alp[2] = 13 * n2 / 48 - 3 * n3 / 5 + 557 * n4 / 1440 + 281 * n5 / 630 - 1983433 * n6 / 1935360;
        alp[3] = 61 * n3 / 240 - 103 * n4 / 140 + 15061 * n5 / 26880 + 167603 * n6 / 181440;
        alp[4] = 49561 * n4 / 161280 - 179 * n5 / 168 + 6601661 * n6 / 7257600;
        alp[5] = 34729 * n5 / 80640 - 3418889 * n6 / 1995840;
        alp[6] = 212378941 * n6 / 319334400;
        // eq. 36
        bet[1] = n / 2 - 2 * n2 / 3 + 37 * n3 / 96 - n4 / 360 - 81 * n5 / 512 + 96199 * n6 / 604800;
        bet[2] = n2 / 48 + n3 / 15 - 437 * n4 / 1440 + 46 * n5 / 105 - 1118711 * n6 / 3870720;
        bet[3] = 17 * n3 / 480 - 37 * n4 / 840 - 209 * n5 / 4480 + 5569 * n6 / 90720;
        bet[4] = 4397 * n4 / 161280 - 11 * n5 / 504 - 830251 * n6 / 7257600;
        bet[5] = 4583 * n5 / 161280 - 108847 * n6 / 3991680;
        bet[6] = 20648693 * n6 / 638668800;
    }
};

const Series &series()
{
    static const Series s;
    return s;
}

// sum_j c[j] sin(2 j z), j = 1..6, by Clenshaw: b_k = c_k + 2 cos(2z) b_{k+1} - b_{k+2}, the sum is b_1 sin(2z)
std::complex<double> clenshaw_sin(const double c[7], std::complex<double> z)
{
    const std::complex<double> two_cos = 2.0 * std::cos(2.0 * z);
    std::complex<double> b1 = 0, b2 = 0;
    for (int k = 6; k >= 1; k--)
    {
        const std::complex<double> b0 = c[k] + two_cos * b1 - b2;
        b2 = b1;
        b1 = b0;
    }
    return b1 * std::sin(2.0 * z);
}

// tan of the conformal latitude from tan of the geographic one (eqs. 7-9)
double taup_of(double tau, double e)
{
    const double t1 = std::hypot(1.0, tau);
    const double sig = std::sinh(e * std::atanh(e * tau / t1));
    return std::hypot(1.0, sig) * tau - sig * t1;
}

// the inverse by Newton's method (eqs. 19-21)
double tau_of(double taup, double e, double e2m)
{
    double tau = taup / e2m;
    if (!std::isfinite(tau))
        return tau;
    for (int i = 0; i < 8; i++)
    {
        const double tp = taup_of(tau, e);
        const double d = (taup - tp) / std::hypot(1.0, tp) * (1 + e2m * tau * tau) / (e2m * std::hypot(1.0, tau));
        tau += d;
        if (!(std::fabs(d) > 1e-17 * std::fmax(1.0, std::fabs(tau))))
            break;
    }
    return tau;
}

double round_g(double v) // what `ostream << v` prints, read back
{
    char buf[64];
    std::snprintf(buf, sizeof buf, "%g", v);
    return std::strtod(buf, nullptr);
}

void set_nan(double out[3])
{
    out[0] = out[1] = out[2] = NAN;
}

} // namespace

bool GeoCoord::setOrigin(double latitude, double longitude)
{
    _init = false;
    _origin_lat = latitude;
    _origin_lon = longitude;
    if (!std::isfinite(latitude) || !std::isfinite(longitude))
        return false;
    _lat0 = round_g(latitude);
    _lon0 = round_g(longitude);
    if (std::fabs(_lat0) > 90 || std::fabs(_lon0) > 360)
        return false;
    const Series &s = series();
    const double chi0 = std::atan(taup_of(std::tan(_lat0 * DEG), s.e));
    _xi0 = chi0 + clenshaw_sin(s.alp, std::complex<double>(chi0, 0)).real();
    _init = true;
    return true;
}

void GeoCoord::toLocalCS(double latitude, double longitude, double altitude, double out[3]) const
{
    if (!_init || !std::isfinite(latitude) || !std::isfinite(longitude) || !std::isfinite(altitude) || std::fabs(latitude) > 90)
        return set_nan(out);
    double dl = std::remainder(longitude - _lon0, 360.0);
    if (!(std::fabs(dl) < 90))
        return set_nan(out);
    const Series &s = series();
    const double lam = dl * DEG;
    const double taup = taup_of(std::tan(latitude * DEG), s.e);
    const double cl = std::cos(lam), sl = std::sin(lam);
    const std::complex<double> zp(std::atan2(taup, cl), std::asinh(sl / std::hypot(taup, cl)));
    const std::complex<double> z = zp + clenshaw_sin(s.alp, zp);
    out[0] = s.A * z.imag();
    out[1] = s.A * (z.real() - _xi0);
    out[2] = altitude;
    if (!std::isfinite(out[0]) || !std::isfinite(out[1]))
        set_nan(out);
}

void GeoCoord::toWGS84(const double local[3], double out[3]) const
{
    if (!_init || !std::isfinite(local[0]) || !std::isfinite(local[1]) || !std::isfinite(local[2]))
        return set_nan(out);
    const Series &s = series();
    const std::complex<double> z(local[1] / s.A + _xi0, local[0] / s.A);
    if (std::fabs(z.imag()) > 20) // sinh would overflow long before anything on the ellipsoid is reached
        return set_nan(out);
    const std::complex<double> zp = z - clenshaw_sin(s.bet, z);
    const double sh = std::sinh(zp.imag()), c = std::cos(zp.real());
    const double taup = std::sin(zp.real()) / std::hypot(sh, c);
    const double lam = std::atan2(sh, c);
    const double lat = std::atan(tau_of(taup, s.e, s.e2m)) / DEG;
    double lon = _lon0 + lam / DEG;
    if (lon >= 180)
        lon -= 360;
    else if (lon < -180)
        lon += 360;
    if (!std::isfinite(lat) || !std::isfinite(lon))
        return set_nan(out);
    out[0] = lon;
    out[1] = lat;
    out[2] = local[2];
}

std::string GeoCoord::getWKT() const
{
    if (!_init)
        return "UNKNOWN";
    char lat[64], lon[64];
    std::snprintf(lat, sizeof lat, "%g", _origin_lat);
    std::snprintf(lon, sizeof lon, "%g", _origin_lon);
    return std::string("PROJCS[\"Custom Transverse Mercator\",\n"
                       "    GEOGCS[\"WGS 84\",\n"
                       "        DATUM[\"WGS_1984\",\n"
                       "            SPHEROID[\"WGS 84\",6378137,298.257223563,\n"
                       "                AUTHORITY[\"EPSG\",\"7030\"]],\n"
                       "            AUTHORITY[\"EPSG\",\"6326\"]],\n"
                       "        PRIMEM[\"Greenwich\",0,\n"
                       "            AUTHORITY[\"EPSG\",\"8901\"]],\n"
                       "        UNIT[\"degree\",0.0174532925199433,\n"
                       "            AUTHORITY[\"EPSG\",\"9122\"]],\n"
                       "        AUTHORITY[\"EPSG\",\"4326\"]],\n"
                       "    PROJECTION[\"Transverse_Mercator\"],\n"
                       "    PARAMETER[\"latitude_of_origin\",") +
           lat +
           "],\n"
           "    PARAMETER[\"central_meridian\"," +
           lon +
           "],\n"
           "    PARAMETER[\"scale_factor\",1],\n"
           "    PARAMETER[\"false_easting\",0],\n"
           "    PARAMETER[\"false_northing\",0],\n"
           "    UNIT[\"metre\",1,\n"
           "        AUTHORITY[\"EPSG\",\"9001\"]],\n"
           "    AXIS[\"Easting\",EAST],\n"
           "    AXIS[\"Northing\",NORTH]]";
}

} // namespace opencalibration_amd
