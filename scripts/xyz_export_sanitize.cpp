// Stand-alone check of the point cloud export's host code (csrc/xyz_export.hpp, csrc/host/xyz_export.hpp; DESIGN.md section
// 4.16) under AddressSanitizer and UndefinedBehaviorSanitizer: host code only, its own main, no device, no library.
//
//   g++ -std=c++17 -O1 -g -fopenmp -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       scripts/xyz_export_sanitize.cpp -o /tmp/xyz_export_sanitize && /tmp/xyz_export_sanitize
//
//   * the integer formatter and the host formatter over the tests' families of numbers (random bit patterns over the covered
//     binades, uniform coordinates, half-way cases with both neighbours, multiples of half a unit of the sixth digit, the
//     edges, the values left to snprintf) against `ostream << double`; every number is written a second time into a heap
//     block of exactly its length;
//   * outlier boxes and cloud texts of random clouds (empty, one point, one cell, flat, with far points, with numbers left
//     to snprintf) with the cloud, the box and the text each in a heap block of exactly its size, against std::map counts and
//     an ostringstream;
//   * the refusals: a NaN, an infinity, 2^63 and -2^63 as a coordinate.
#include "../opencalibration_amd/csrc/host/xyz_export.hpp"

#include <cmath>
#include <cstdlib>
#include <memory>
#include <random>
#include <sstream>

using namespace opencalibration_amd;

namespace
{

int failures = 0;
size_t numbers = 0, clouds = 0, points = 0;

void expect(bool ok, const char *what, double v = 0)
{
    if (!ok)
    {
        std::fprintf(stderr, "FAILED: %s (%.17g)\n", what, v);
        failures++;
    }
}

std::string ostream_text(double v)
{
    std::ostringstream s;
    s << v;
    return s.str();
}

void check_number(double v)
{
    numbers++;
    const std::string want = ostream_text(v);
    std::unique_ptr<char[]> room(new char[ochip_xe::NUMBER_CHARS]);
    const int own = ochip_xe::format_g6(v, room.get());
    const double a = std::fabs(v);
    const bool covered = a == 0 || (a >= 1e-5 && a < 9223372036854775808.0);
    expect((own != 0) == covered, "the integer formatter covers exactly 0 and [1e-5, 2^63)", v);
    if (own)
    {
        expect(std::string(room.get(), own) == want, "format_g6 != ostream", v);
        std::unique_ptr<char[]> exact(new char[own]); // a write past the number's own length is a report
        expect(ochip_xe::format_g6(v, exact.get()) == own && std::string(exact.get(), own) == want, "format_g6 into an exact block", v);
    }
    const int any = xyz_host::format_number(v, room.get());
    expect(any > 0 && any <= 13 && std::string(room.get(), any) == want, "format_number != ostream", v);
}

double from_bits(uint64_t b)
{
    double v;
    std::memcpy(&v, &b, 8);
    return v;
}

void check_cloud(const std::vector<double> &cloud, bool must_refuse = false)
{
    clouds++;
    const size_t n = cloud.size() / 3;
    points += n;
    std::unique_ptr<double[]> xyz(new double[cloud.size()]);
    if (!cloud.empty())
        std::memcpy(xyz.get(), cloud.data(), cloud.size() * 8);
    std::unique_ptr<int64_t[]> box(new int64_t[6]);
    std::string why;
    const bool ok = xyz_host::outlier_bounds(xyz.get(), n, box.get(), &why);
    if (must_refuse)
    {
        expect(!ok && !why.empty(), "a coordinate without a cell is refused");
        return;
    }
    expect(ok, "outlier_bounds refused a cloud it should take");
    // the yardstick: std::map counts, the walk, an ostringstream
    int64_t want[6];
    for (int a = 0; a < 3; a++)
    {
        std::map<int64_t, uint64_t> cells;
        for (size_t i = 0; i < n; i++)
            cells[static_cast<int64_t>(cloud[3 * i + a])]++;
        std::vector<int64_t> keys;
        std::vector<uint64_t> counts;
        for (const auto &kc : cells)
            keys.push_back(kc.first), counts.push_back(kc.second);
        std::unique_ptr<int64_t[]> k(new int64_t[keys.size()]);
        std::unique_ptr<uint64_t[]> c(new uint64_t[counts.size()]);
        for (size_t r = 0; r < keys.size(); r++)
            k[r] = keys[r], c[r] = counts[r];
        const auto b = ochip_xe::dimbox(k.get(), c.get(), keys.size(), n);
        want[2 * a] = b.first, want[2 * a + 1] = b.second;
    }
    expect(std::memcmp(want, box.get(), sizeof want) == 0, "the box differs from the std::map route");
    for (int filtered = 0; filtered < 2; filtered++)
    {
        const bool off = !filtered || (want[0] == want[1] && want[2] == want[3] && want[4] == want[5]);
        std::ostringstream yard;
        uint64_t kept = 0;
        for (size_t i = 0; i < n; i++)
        {
            bool in = true;
            for (int a = 0; a < 3 && !off; a++)
                in = in && (double)want[2 * a] < cloud[3 * i + a] && cloud[3 * i + a] < (double)want[2 * a + 1];
            if (in)
                yard << cloud[3 * i] << "," << cloud[3 * i + 1] << "," << cloud[3 * i + 2] << "\n", kept++;
        }
        xyz_host::CloudText t;
        t.prepare(xyz.get(), n, filtered ? box.get() : nullptr);
        std::unique_ptr<char[]> text(new char[t.bytes]);
        t.fill(text.get());
        expect(t.kept == kept && std::string(text.get(), t.bytes) == yard.str(), "the text differs from the ostringstream's");
    }
}

} // namespace

int main()
{
    std::mt19937_64 rng(7);
    for (int i = 0; i < 300000; i++)
    {
        const uint64_t r = rng();
        check_number(from_bits((r & 0x800FFFFFFFFFFFFFull) | ((uint64_t)(1023 - 17 + (r >> 52) % 80) << 52)));
    }
    std::uniform_real_distribution<double> coordinate(-2000, 2000);
    for (int i = 0; i < 200000; i++)
        check_number(coordinate(rng));
    for (int j = -3; j <= 9; j++)
        for (int i = 0; i < 6000; i++)
        {
            const double half = ((double)(rng() % 1000000) + 0.5) / std::pow(10.0, j);
            check_number(half), check_number(std::nextafter(half, 0)), check_number(std::nextafter(half, 1e300)), check_number(-half);
        }
    for (int j = -4; j <= 18; j++)
        for (int i = 0; i < 6000; i++)
            check_number((double)(200000 + rng() % 1800000) * 0.5 * std::pow(10.0, j) / 1e6);
    const double edges[] = {0.0, -0.0, 999999.5, 999999.49999999994, 99999.95, 0.0001, 9.9999949999e-5, 2.5e-5, 1e6, 1e15, 123456.5,
                            9.2e18, 1e-5, 1e-7, 1e300, -1e300, 5e-324, -5e-324, 2.2250738585072014e-308, 9223372036854775808.0,
                            18446744073709551616.0, -1.7976931348623157e308, std::nextafter(1e-5, 0), std::nextafter(9223372036854775808.0, 0),
                            HUGE_VAL, -HUGE_VAL};
    for (double v : edges)
        check_number(v);

    std::normal_distribution<double> height(-48, 1.5), spread(0, 400);
    for (size_t n : {(size_t)0, (size_t)1, (size_t)39, (size_t)40, (size_t)64, (size_t)257, (size_t)5000})
        for (int kind = 0; kind < 5; kind++)
        {
            std::vector<double> c;
            std::uniform_real_distribution<double> wide(-120, 120), cell(3.1, 3.9);
            for (size_t i = 0; i < n; i++)
            {
                if (kind == 1) // one integer cell
                    c.insert(c.end(), {cell(rng), cell(rng), cell(rng)});
                else if (kind == 2) // flat in z
                    c.insert(c.end(), {wide(rng), wide(rng), 5.5});
                else if (i % 97 == 5) // a far point
                    c.insert(c.end(), {spread(rng), spread(rng), spread(rng)});
                else
                    c.insert(c.end(), {wide(rng), wide(rng), height(rng)});
            }
            if (kind == 3 && n > 2)
                c[3] = 1e12, c[7] = -1e-7, c[8] = 5e-324; // a wide span and two numbers left to snprintf
            if (kind == 4 && n > 2)
                c[0] = -0.9, c[3] = 0.9, c[6] = -0.0;
            check_cloud(c);
        }
    for (double bad : {(double)NAN, (double)HUGE_VAL, (double)-HUGE_VAL, 9223372036854775808.0, -9223372036854775808.0, 1e300})
        check_cloud({1.0, 2.0, 3.0, 4.0, bad, 6.0, 7.0, 8.0, 9.0}, true);

    std::printf("%zu numbers, %zu clouds with %zu points: %d failures\n", numbers, clouds, points, failures);
    return failures != 0;
}
