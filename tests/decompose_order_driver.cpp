// Stand-alone checks of csrc/decompose.hpp on the host (tests/test_decompose_oracle.py builds and runs it, under the address
// and undefined-behaviour sanitizers where their runtimes link):
//   order_by_votes against std::stable_sort with the reference's non-strict comparator `score >=` on all 625 score rows of
//   {-1, 0, 1, 2, 3}^4 - the comparator is no strict weak order, so what the sort leaves is libstdc++'s behaviour, and the
//   header's restatement has to be that behaviour;
//   quaternion_from_rotation on all four branches of Shoemake's method (trace > 0, and each diagonal entry the largest),
//   rotations by exactly pi included, against the rotation rebuilt from the quaternion.
#include "../opencalibration_amd/csrc/decompose.hpp"

#include <algorithm>
#include <array>
#include <cstdio>
#include <cstdlib>

namespace
{
struct rec
{
    int score, index;
};

int check_orders()
{
    static const int values[5] = {-1, 0, 1, 2, 3};
    int rows = 0, ties_kept_reversed = 0;
    for (int a = 0; a < 5; a++)
        for (int b = 0; b < 5; b++)
            for (int c = 0; c < 5; c++)
                for (int d = 0; d < 5; d++)
                {
                    const int score[4] = {values[a], values[b], values[c], values[d]};
                    std::array<rec, 4> r;
                    for (int i = 0; i < 4; i++)
                        r[i] = rec{score[i], i};
                    std::stable_sort(r.begin(), r.end(), [](const rec &p1, const rec &p2) { return p1.score >= p2.score; });
                    int order[4];
                    ochip_dc::order_by_votes(score, order);
                    for (int k = 0; k < 4; k++)
                        if (order[k] != r[k].index)
                        {
                            std::printf("order_by_votes (%d %d %d %d): %d %d %d %d, std::stable_sort %d %d %d %d\n", score[0], score[1],
                                        score[2], score[3], order[0], order[1], order[2], order[3], r[0].index, r[1].index, r[2].index,
                                        r[3].index);
                            return 1;
                        }
                    // what the tests of the poses rely on: score descending, equal scores in descending solution index
                    for (int k = 0; k + 1 < 4; k++)
                    {
                        const int s0 = score[order[k]], s1 = score[order[k + 1]];
                        if (s0 < s1 || (s0 == s1 && order[k] < order[k + 1]))
                        {
                            std::printf("order of (%d %d %d %d) is not score descending, index descending\n", score[0], score[1], score[2],
                                        score[3]);
                            return 1;
                        }
                        ties_kept_reversed += s0 == s1;
                    }
                    rows++;
                }
    std::printf("orders: %d rows equal std::stable_sort, %d tied neighbours in descending index\n", rows, ties_kept_reversed);
    return rows == 625 ? 0 : 1;
}

ochip_dc::M3 rotation_of(const double q[4]) // x y z w, any norm
{
    const double n = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
    const double x = q[0], y = q[1], z = q[2], w = q[3], s = 2 / n;
    ochip_dc::M3 m;
    m.a[0][0] = 1 - s * (y * y + z * z), m.a[0][1] = s * (x * y - z * w), m.a[0][2] = s * (x * z + y * w);
    m.a[1][0] = s * (x * y + z * w), m.a[1][1] = 1 - s * (x * x + z * z), m.a[1][2] = s * (y * z - x * w);
    m.a[2][0] = s * (x * z - y * w), m.a[2][1] = s * (y * z + x * w), m.a[2][2] = 1 - s * (x * x + y * y);
    return m;
}

int branch_of(const ochip_dc::M3 &m) // 3: trace > 0, else the index of the largest diagonal entry (the first on a tie)
{
    if (m.a[0][0] + m.a[1][1] + m.a[2][2] > 0)
        return 3;
    int i = 0;
    if (m.a[1][1] > m.a[0][0])
        i = 1;
    if (m.a[2][2] > m.a[i][i])
        i = 2;
    return i;
}

int seen[4], seen_pi[3];

int check_quaternion(const ochip_dc::M3 &R, const char *what, bool is_pi)
{
    double q[4];
    ochip_dc::quaternion_from_rotation(R, q);
    const double n = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    const ochip_dc::M3 back = rotation_of(q);
    double worst = std::fabs(n - 1);
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++)
            worst = std::fmax(worst, std::fabs(back.a[i][j] - R.a[i][j]));
    // R is a rotation to a few ulp (built from a quaternion in fp64); Shoemake's divisor is at least 1 on the branch taken
    if (!(worst <= 16 * 2.220446049250313e-16))
    {
        std::printf("quaternion_from_rotation, %s: R(q) differs from R by %.3g (q = %.17g %.17g %.17g %.17g)\n", what, worst, q[0], q[1],
                    q[2], q[3]);
        return 1;
    }
    const int b = branch_of(R);
    seen[b]++;
    if (is_pi && b < 3)
        seen_pi[b]++;
    return 0;
}

int check_quaternions()
{
    unsigned long long state = 0x9E3779B97F4A7C15ull;
    auto uniform = [&]() { // xorshift64*, in (-1, 1)
        state ^= state >> 12, state ^= state << 25, state ^= state >> 27;
        return (double)((state * 0x2545F4914F6CDD1Dull) >> 11) / 4503599627370496.0 - 1.0;
    };
    for (int k = 0; k < 4000; k++)
    {
        double q[4] = {uniform(), uniform(), uniform(), uniform()};
        if (k % 2)
            q[3] *= 1e-3; // angles near pi: trace <= 0, the three diagonal branches
        if (q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3] < 1e-3)
            continue;
        if (check_quaternion(rotation_of(q), "drawn", false))
            return 1;
    }
    // rotations by exactly pi: about the three axes (exact matrices: diag(1, -1, -1) and its kin), and about drawn axes
    // (w = 0 exactly), the largest component in every position
    for (int axis = 0; axis < 3; axis++)
    {
        double q[4] = {0, 0, 0, 0};
        q[axis] = 1;
        if (check_quaternion(rotation_of(q), "pi about an axis", true))
            return 1;
        for (int k = 0; k < 200; k++)
        {
            double p[4] = {0.7 * uniform(), 0.7 * uniform(), 0.7 * uniform(), 0};
            p[axis] = p[axis] < 0 ? -1 : 1;
            if (check_quaternion(rotation_of(p), "pi about a drawn axis", true))
                return 1;
        }
    }
    // the edge of the first branch: trace exactly 0 (120 degrees about (1, 1, 1) is a permutation matrix) goes to the diagonal
    // branches, and the identity
    {
        const double q120[4] = {0.5, 0.5, 0.5, 0.5}, qid[4] = {0, 0, 0, 1};
        const ochip_dc::M3 P = rotation_of(q120);
        if (P.a[0][0] + P.a[1][1] + P.a[2][2] != 0 || branch_of(P) != 0)
        {
            std::printf("the permutation matrix does not have trace 0\n");
            return 1;
        }
        if (check_quaternion(P, "trace 0", false) || check_quaternion(rotation_of(qid), "identity", false))
            return 1;
    }
    std::printf("quaternions: trace > 0 %d, diagonal 0 / 1 / 2 largest %d / %d / %d, of them by exactly pi %d / %d / %d\n", seen[3], seen[0],
                seen[1], seen[2], seen_pi[0], seen_pi[1], seen_pi[2]);
    for (int b = 0; b < 4; b++)
        if (seen[b] < 100 || (b < 3 && seen_pi[b] < 100))
        {
            std::printf("branch %d is not covered\n", b);
            return 1;
        }
    return 0;
}
} // namespace

int main()
{
    if (check_orders() || check_quaternions())
        return 1;
    std::printf("clean\n");
    return 0;
}
