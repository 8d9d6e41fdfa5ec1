// GeoCoord (include/opencalibration/geo_coord/geo_coord.hpp, src/geo_coord/geo_coord.cpp): the survey's local frame, a
// Transverse Mercator on the WGS84 ellipsoid about the first image's position - k0 = 1, no false origin, northing measured
// from latitude_of_origin.  The reference hands a WKT to PROJ; PROJ is not here, so the projection is restated: Krueger's
// series to n^6 in both directions (Karney 2011, eqs. 7-11, 35, 36), the sums by Clenshaw's recurrence, all in fp64.
//
// The reference writes its WKT with `ostream << latitude`, six significant digits, so what PROJ projects about is %g of
// the origin while getOriginLatitude() keeps the unrounded number: `origin_*` is the latter, `centre_*` the former.
#pragma once

#include <cstddef>
#include <string>

namespace opencalibration_amd
{

class GeoCoord
{
  public:
    GeoCoord() = default;
    bool setOrigin(double latitude, double longitude); // false (and uninitialised) on a non-finite or out-of-range origin
    bool isInitialized() const
    {
        return _init;
    }
    double getOriginLatitude() const
    {
        return _origin_lat;
    }
    double getOriginLongitude() const
    {
        return _origin_lon;
    }
    double centreLatitude() const // strtod("%g") of the origin: what the projection is about
    {
        return _lat0;
    }
    double centreLongitude() const
    {
        return _lon0;
    }
    // (latitude, longitude, altitude) -> (easting, northing, altitude); NaN NaN NaN where the reference's transform fails:
    // uninitialised, non-finite input, |latitude| > 90, 90 degrees or more from the central meridian (geo_coord.cpp:110)
    void toLocalCS(double latitude, double longitude, double altitude, double out[3]) const;
    // (easting, northing, altitude) -> (longitude, latitude, altitude), the traditional GIS order the reference asks for
    void toWGS84(const double local[3], double out[3]) const;
    std::string getWKT() const; // the text setOrigin builds (geo_coord.cpp:42-67); "UNKNOWN" when uninitialised

  private:
    bool _init = false;
    double _origin_lat = 0, _origin_lon = 0, _lat0 = 0, _lon0 = 0;
    double _xi0 = 0; // the rectifying latitude of _lat0: northing = A (xi - xi0)
};

} // namespace opencalibration_amd
