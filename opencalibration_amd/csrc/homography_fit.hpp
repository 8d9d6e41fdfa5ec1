// homography_model on the device (src/model_inliers/homography_model.cpp:19-136), one wavefront per pair (gfx950): the model
// and its symmetric transfer error, fit (the wave-cooperative full_piv_lu_solve9, and lane_fit - a private 9 x 9 system per
// lane - for the homography loop's fast-forward), fitInliers (regen_lu_solve9 through fit_inliers) and checkSampleDegeneracy.
// Eigen's FullPivLU is restated from its algorithm.  Used by the homography loop and the refit (ransac.hip) and by the
// fundamental-matrix model's DEGENSAC (ransac_epipolar.hip).  The three factorisations are held at their edges against the
// oracle bit for bit and against a long-double restatement through ochip_refit_homography_batch and the seam
// ochip_debug_homography_fit4 (tests/test_gpu_homography_fit.py).
#pragma once

#include "ransac_loop.hpp"

namespace
{

constexpr int FB = 32; // samples fitted side by side, one per lane, by lane_fit (ransac.hip: fast_forward)

// The pivot search's reduction over the wavefront: the largest value, ties to the smaller (column, row) - the first maximum
// of the column-by-column scan, whatever order the candidates meet in.  Every lane ends with the result.  The six
// butterfly stages used to be four LDS-crossbar shuffles each (__shfl_xor of a double and two indices: 24 dependent
// ds_bpermute per pivot, 9 pivots per hypothesis - the critical path of a kernel that is one wavefront per image pair);
// now the indices travel as one word and the four stages inside a row of 16 lanes are DPP moves (quad permutes, then
// rotations by 4 and 8: any pairing that ends with every lane having met every other serves a commutative, associative
// choice), two stages across the rows remain shuffles.
template <int CTRL> __device__ __forceinline__ uint32_t dpp_word(uint32_t x)
{
    return (uint32_t)__builtin_amdgcn_update_dpp((int)x, (int)x, CTRL, 0xf, 0xf, false);
}
__device__ __forceinline__ void first_maximum_take(double &bv, uint32_t &key, double ov, uint32_t ok)
{
    if (ov > bv || (ov == bv && ok < key))
    {
        bv = ov;
        key = ok;
    }
}
template <int CTRL> __device__ __forceinline__ void first_maximum_stage(double &bv, uint32_t &key)
{
    const unsigned long long bits = (unsigned long long)__double_as_longlong(bv);
    const uint32_t lo = dpp_word<CTRL>((uint32_t)bits), hi = dpp_word<CTRL>((uint32_t)(bits >> 32));
    const uint32_t ok = dpp_word<CTRL>(key);
    first_maximum_take(bv, key, __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo)), ok);
}
__device__ __forceinline__ void wave_first_maximum(double &bv, uint32_t &bi, uint32_t &bj)
{
    uint32_t key = (bj << 28) | bi; // (column, row): a column is below 9 (4 bits), which leaves 28 bits to the row
    first_maximum_stage<0xB1>(bv, key);  // quad_perm [1, 0, 3, 2]
    first_maximum_stage<0x4E>(bv, key);  // quad_perm [2, 3, 0, 1]
    first_maximum_stage<0x124>(bv, key); // row_ror:4
    first_maximum_stage<0x128>(bv, key); // row_ror:8
#pragma unroll
    for (int off = 16; off <= 32; off <<= 1)
        first_maximum_take(bv, key, __shfl_xor(bv, off), __shfl_xor(key, off));
    bi = key & 0x0FFFFFFFu;
    bj = key >> 28;
}

struct model_t // homography_model state, wave-uniform
{
    double H[9], Hi[9];
};

__device__ __forceinline__ void set_nan(model_t &m)
{
    for (int i = 0; i < 9; i++)
        m.H[i] = m.Hi[i] = __builtin_nan("");
}

// Eigen compute_inverse_size3 (cofactors, 1/det) — same order as the restatement
__device__ __forceinline__ double cof(const double *m, int i, int j)
{
    const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
    return m[i1 * 3 + j1] * m[i2 * 3 + j2] - m[i1 * 3 + j2] * m[i2 * 3 + j1];
}

__device__ __forceinline__ void model_from_solution(model_t &m, const double *h) // homography_model.cpp:45-49
{
    const double s = h[8];
    for (int i = 0; i < 9; i++)
        m.H[i] = h[i] / s;
    const double c00 = cof(m.H, 0, 0), c10 = cof(m.H, 1, 0), c20 = cof(m.H, 2, 0);
    const double d = c00 * m.H[0] + c10 * m.H[3] + c20 * m.H[6];
    const double invdet = 1.0 / d;
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++)
            m.Hi[r * 3 + c] = cof(m.H, c, r) * invdet;
}

// homography_model::error (homography_model.cpp:89-97) on pre-divided coordinates (x/z, y/z, z/z == 1)
__device__ __forceinline__ double transfer_error(const model_t &m, double x1, double y1, double x2, double y2)
{
    const double fx_ = m.H[0] * x1 + m.H[1] * y1 + m.H[2] * 1.0;
    const double fy_ = m.H[3] * x1 + m.H[4] * y1 + m.H[5] * 1.0;
    const double fz_ = m.H[6] * x1 + m.H[7] * y1 + m.H[8] * 1.0;
    const double bx_ = m.Hi[0] * x2 + m.Hi[1] * y2 + m.Hi[2] * 1.0;
    const double by_ = m.Hi[3] * x2 + m.Hi[4] * y2 + m.Hi[5] * 1.0;
    const double bz_ = m.Hi[6] * x2 + m.Hi[7] * y2 + m.Hi[8] * 1.0;
    const double fx = fx_ / fz_ - x2, fy = fy_ / fz_ - y2;
    const double bx = bx_ / bz_ - x1, by = by_ / bz_ - y1;
    const double fwd = fx * fx + fy * fy;
    const double bwd = bx * bx + by * by;
    return sqrt((fwd + bwd) / 2.0);
}

// ---- Eigen FullPivLU<Matrix<double, rows, 9>>::solve(e_last).  Pivot search order / ties (column-by-column scan,
//      strict '>'), rank threshold and substitution order are the restated Eigen algorithm of the oracle.
struct lu_state
{
    uint32_t rowT[9], colT[9];
    uint32_t nonzero_pivots;
    double maxpivot;
};

// rank, then the solve steps on the factored leading 9 x 9 block B (column-major, ld 9, in LDS); uniform work
__device__ void lu_finish(const double *B, uint32_t rows, uint32_t size, const lu_state &st, double *sol /*[9], uniform*/)
{
    const uint32_t ld = 9;
    const double premult = fabs(st.maxpivot) * (2.220446049250313e-16 * (double)size);
    uint32_t rank = 0;
    for (uint32_t i = 0; i < st.nonzero_pivots; i++)
        rank += (fabs(B[(size_t)i * ld + i]) > premult) ? 1 : 0;
    for (int i = 0; i < 9; i++)
        sol[i] = 0;
    if (rank == 0)
        return;
    // c = P * e_last: follow the single 1 through the row transpositions
    uint32_t pos = rows - 1;
    for (uint32_t k = 0; k < size; k++)
    {
        if (pos == k)
            pos = st.rowT[k];
        else if (pos == st.rowT[k])
            pos = k;
    }
    double c[9];
    for (uint32_t i = 0; i < 9; i++)
        c[i] = (i == pos) ? 1.0 : 0.0;
    for (uint32_t j = 0; j < size; j++) // unit-lower forward substitution, column oriented
    {
        const double cj = c[j];
        for (uint32_t i = j + 1; i < size; i++)
            c[i] -= cj * B[(size_t)j * ld + i];
    }
    for (uint32_t jj = rank; jj-- > 0;) // upper back substitution, column oriented
    {
        c[jj] /= B[(size_t)jj * ld + jj];
        const double cj = c[jj];
        for (uint32_t i = 0; i < jj; i++)
            c[i] -= cj * B[(size_t)jj * ld + i];
    }
    uint32_t perm[9] = {0, 1, 2, 3, 4, 5, 6, 7, 8};
    for (uint32_t k = 0; k < size; k++)
    {
        const uint32_t t = perm[k];
        perm[k] = perm[st.colT[k]];
        perm[st.colT[k]] = t;
    }
    for (uint32_t i = 0; i < rank; i++)
        sol[perm[i]] = c[i];
}

// The minimal-sample fit: A is the 9 x 9 system in LDS (ld 9), rows <= 9; the wave cooperates, lanes over rows.
__device__ void full_piv_lu_solve9(double *A, uint32_t rows, double *sol /*[9], uniform*/)
{
    const int lane = threadIdx.x;
    const uint32_t cols = 9, ld = 9;
    const uint32_t size = rows < cols ? rows : cols;
    lu_state st;
    st.nonzero_pivots = size;
    st.maxpivot = 0;

    for (uint32_t k = 0; k < size; k++)
    {
        __syncthreads();
        // ---- pivot search over the bottom-right corner
        double bv = -1.0;
        uint32_t bi = k, bj = k;
        for (uint32_t j = k; j < cols; j++)
            for (uint32_t i = k + lane; i < rows; i += W)
            {
                const double v = fabs(A[(size_t)j * ld + i]);
                if (v > bv) // within a lane (j, i) ascend, so strict '>' keeps the first maximum
                {
                    bv = v;
                    bi = i;
                    bj = j;
                }
            }
        wave_first_maximum(bv, bi, bj);
        const double akk = A[(size_t)k * ld + k];
        if (akk != akk) // a NaN in the first scanned cell sticks (nothing compares greater than NaN)
        {
            bv = akk;
            bi = k;
            bj = k;
        }
        else if (bv < 0) // every candidate was NaN except none: keep (k,k)
        {
            bv = fabs(akk);
            bi = k;
            bj = k;
        }
        if (bv == 0.0)
        {
            st.nonzero_pivots = k;
            for (uint32_t i = k; i < size; i++)
            {
                st.rowT[i] = i;
                st.colT[i] = i;
            }
            break;
        }
        if (bv > st.maxpivot)
            st.maxpivot = bv;
        st.rowT[k] = bi;
        st.colT[k] = bj;
        // ---- row swap k <-> bi (lanes over the 9 columns), then column swap k <-> bj (lanes over rows)
        if (k != bi && lane < (int)cols)
        {
            const double t = A[(size_t)lane * ld + k];
            A[(size_t)lane * ld + k] = A[(size_t)lane * ld + bi];
            A[(size_t)lane * ld + bi] = t;
        }
        __syncthreads();
        if (k != bj)
            for (uint32_t i = lane; i < rows; i += W)
            {
                const double t = A[(size_t)k * ld + i];
                A[(size_t)k * ld + i] = A[(size_t)bj * ld + i];
                A[(size_t)bj * ld + i] = t;
            }
        __syncthreads();
        // ---- eliminate: col(k).tail /= pivot; block(k+1,k+1) -= col(k).tail * row(k).tail
        const double p = A[(size_t)k * ld + k];
        double rowk[9];
        for (uint32_t j = k + 1; j < cols; j++)
            rowk[j] = A[(size_t)j * ld + k];
        __syncthreads();
        if (k < rows - 1)
            for (uint32_t i = k + 1 + lane; i < rows; i += W)
            {
                const double l = A[(size_t)k * ld + i] / p;
                A[(size_t)k * ld + i] = l;
                if (k < size - 1)
                    for (uint32_t j = k + 1; j < cols; j++)
                        A[(size_t)j * ld + i] -= l * rowk[j];
            }
    }
    __syncthreads();
    lu_finish(A, rows, size, st, sol);
}

// ---- the tall (2n+1) x 9 system of fitInliers (rows > 9): the same factorisation
struct piv_t
{
    double v;
    uint32_t i, j;
};
__device__ __forceinline__ void piv_reduce(piv_t &b)
{
    wave_first_maximum(b.v, b.i, b.j);
}

// ---- Round 5: the factorisation of the tall system WITHOUT the system.  Rounds 2 - 4 kept it column-major in HBM and went
//      over it once per elimination step: the (2 n + 1) x 9 matrix of a pair (170 KB at 1 180 matches) read and written
//      once per elimination step, 2.4 factorisations per pair, 2 048 pairs resident - 40 GB per 9 000-pair launch, 59 % of
//      the kernel's cycles.  A row of the system is a function of its correspondence's four coordinates, and what the
//      eliminations do to a row depends on nothing but the row and the pivot rows so far (which ARE the U part of the
//      factored leading block, 81 doubles in LDS).  So step k regenerates every row from its coordinates, applies the k
//      eliminations so far - the float operations of the stored form in its order, column for column - and looks for the
//      next pivot among the results; nothing is written.  36 eliminations per row instead of 9, 33 bytes read per
//      correspondence and step instead of ~1 600 per factorisation step.
//      Bookkeeping.  Positions: a row that never took part in a row transposition stands where it started (2 rank + a/b);
//      the rows that did - the nine that start in the leading block, every pivot row, the last row (0 .. 0 1), and the sibling
//      of a pivot row - live in a table of at most 29 entries in LDS with their position, and the sweep over the
//      correspondences skips them (rank < 5, or one of the <= 9 correspondences a pivot came from).  Columns: sigma maps
//      position -> original column (a nibble each); the U rows in LDS are kept in the current arrangement, so a regenerated
//      row is permuted once and every elimination is the stored form's.
__device__ __forceinline__ uint32_t nib_get(uint64_t p, uint32_t k)
{
    return (uint32_t)(p >> (4 * k)) & 15u;
}
__device__ __forceinline__ uint64_t nib_set(uint64_t p, uint32_t k, uint32_t v)
{
    return (p & ~(15ull << (4 * k))) | ((uint64_t)v << (4 * k));
}
typedef double dvec16 __attribute__((ext_vector_type(16))); // (indexed by a wave-uniform value: s_set_gpr_idx, no select chain)

struct tall_tab
{
    double xy[32][4];      // x, y, x', y' of the entry's correspondence
    uint32_t pos[32];      // where the row stands now
    uint32_t kind[32];     // 0 / 1: first / second row of its correspondence, 2: the last row; | 4: a pivot row (done)
    uint32_t top[9];       // entry at position 0 .. 8
    uint32_t piv_match[9]; // correspondence whose two rows entered the table at step t (~0u: none did)
    uint32_t n;
};
typedef __attribute__((address_space(3))) tall_tab lds_tab;
typedef __attribute__((address_space(3))) double lds_double;
typedef const __attribute__((address_space(3))) double lds_cdouble;
typedef const __attribute__((address_space(1))) double glb_cdouble;
typedef const __attribute__((address_space(1))) uint8_t glb_cbyte;
struct regen_in // what the factorisation reads of a pair, in global memory
{
    glb_cdouble *x1, *y1, *x2, *y2;
    glb_cbyte *inl;
    uint32_t M;
};

// A row of the system has eight values to draw from - write_dlt_rows' {-x, -y, -1, 0, x x', y x', x'} (second row: y' for x') and
// the last row's 1 - and a map from column to value: 0x654333210 / 0x654210333 / 0x733333333, a nibble per column.
typedef double dvec8 __attribute__((ext_vector_type(8)));
__device__ __forceinline__ dvec8 dlt_values(double x, double y, double xp)
{
    dvec8 o;
    o[0] = -x, o[1] = -y, o[2] = -1.0, o[3] = 0.0, o[4] = x * xp, o[5] = y * xp, o[6] = xp, o[7] = 1.0;
    return o;
}
__device__ __forceinline__ unsigned long long dlt_map(uint32_t kind)
{
    return kind == 0 ? 0x654333210ull : (kind == 1 ? 0x654210333ull : 0x733333333ull);
}

// a row in position order from its values.  `pick` = the value index of every position, a nibble each (wave-uniform: sigma
// through the row kind's map)
__device__ __forceinline__ void row_pick(const dvec8 &o, uint32_t pick_lo, uint32_t pick_hi, double (&v)[9])
{
#pragma unroll
    for (int pos = 0; pos < 9; pos++)
        v[pos] = o[pos < 8 ? (pick_lo >> (4 * pos)) & 7u : pick_hi & 7u];
}
// NR rows after K eliminations: v[t] for t < K becomes the row's multiplier of step t (what the stored form leaves in
// column t), v[K ..] the values the search for pivot K looks at.  The U row of the next step is requested while this
// step's arithmetic runs and no further ahead (left to itself the compiler asks for all 44 entries first: 88 registers)
// The multiplier v / p is a true division: what the compiler emits for one is v_div_scale x 2, v_rcp, four fma on the
// reciprocal, a product, a residual, v_div_fmas, v_div_fixup.  The reciprocal chain depends on p alone - wave-uniform here, one
// chain per step and trip instead of one per row - and when neither operand is near the ends of the exponent range
// v_div_scale passes both through, v_div_fmas is an fma and v_div_fixup sets the sign of the operands on the magnitude
// (also for a zero numerator): the FAST form below.  |v| <= |p| (full pivoting), so "near the ends" is: p outside
// [2^-100, 2^100] or not finite, or 0 < |v| < 2^-900; any lane that sees one reports it and the trip's rows are done
// again with the plain division.
__device__ __forceinline__ double refined_reciprocal(double p)
{
    const double r0 = __builtin_amdgcn_rcp(p);
    const double e0 = __builtin_fma(-p, r0, 1.0);
    const double r1 = __builtin_fma(r0, e0, r0);
    const double e1 = __builtin_fma(-p, r1, 1.0);
    return __builtin_fma(r1, e1, r1);
}
__device__ __forceinline__ double divide_in_range(double v, double p, double r2)
{
    const double q0 = v * r2;
    const double e2 = __builtin_fma(-p, q0, v);
    const double q1 = __builtin_fma(e2, r2, q0);
    const unsigned long long qb = (unsigned long long)__double_as_longlong(q1);
    const uint32_t sign = ((uint32_t)((unsigned long long)__double_as_longlong(v) >> 32) ^ (uint32_t)((unsigned long long)__double_as_longlong(p) >> 32)) & 0x80000000u;
    const uint32_t hi = ((uint32_t)(qb >> 32) & 0x7FFFFFFFu) | sign;
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | (qb & 0xFFFFFFFFull)));
}
template <int K, int NR, bool FAST>
__device__ __forceinline__ bool rows_eliminate(lds_cdouble *T9, double (&v)[NR][9])
{
    bool out_of_range = false;
    if (K == 0)
        return out_of_range;
    double u[9];
#pragma unroll
    for (int j = 0; j < 9; j++)
        u[j] = T9[j * 9];
#pragma unroll
    for (int t = 0; t < K; t++)
    {
        double nu[9];
#pragma unroll
        for (int j = 0; j < 9; j++)
            nu[j] = (t + 1 < K && j > t) ? T9[j * 9 + t + 1] : 0.0;
        asm volatile("" ::: "memory");
        const double p = u[t];
        double r2 = 0.0;
        if (FAST)
        {
            r2 = refined_reciprocal(p);
            out_of_range |= !((int)(fabs(p) >= 0x1p-100) & (int)(fabs(p) <= 0x1p100)); // (no short circuit: straight-line code)
        }
#pragma unroll
        for (int r = 0; r < NR; r++)
        {
            if (FAST)
                out_of_range |= (bool)((int)(fabs(v[r][t]) < 0x1p-900) & (int)(v[r][t] != 0.0));
            const double l = FAST ? divide_in_range(v[r][t], p, r2) : v[r][t] / p;
            v[r][t] = l;
#pragma unroll
            for (int j = t + 1; j < 9; j++)
                v[r][j] = v[r][j] - l * u[j];
        }
#pragma unroll
        for (int j = 0; j < 9; j++)
            u[j] = nu[j];
    }
    return out_of_range;
}
// sigma (position -> column) through a kind's map (column -> value): position -> value
__device__ __forceinline__ void compose_pick(uint32_t kind, uint32_t sig_lo, uint32_t sig_hi, uint32_t *pick_lo, uint32_t *pick_hi)
{
    const unsigned long long m = dlt_map(kind);
    uint32_t lo = 0;
#pragma unroll
    for (int pos = 0; pos < 8; pos++)
        lo |= (uint32_t)((m >> (4 * ((sig_lo >> (4 * pos)) & 15u))) & 15ull) << (4 * pos);
    *pick_lo = lo;
    *pick_hi = (uint32_t)((m >> (4 * (sig_hi & 15u))) & 15ull);
}

// the row's first maximum among positions K .. 8 (columns ascend, strict '>': the earliest column of the largest value;
// NaN never wins), offered to the lane's running first maximum
template <int K>
__device__ __forceinline__ bool row_offer(const double (&v)[9], uint32_t pos, piv_t &pv)
{
    double bv = -1.0;
    uint32_t bj = K;
#pragma unroll
    for (int j = K; j < 9; j++)
    {
        const double a = fabs(v[j]);
        if (a > bv)
        {
            bv = a;
            bj = j;
        }
    }
    const bool better = bv >= 0 && (bv > pv.v || (bv == pv.v && (bj < pv.j || (bj == pv.j && pos < pv.i))));
    if (better)
    {
        pv.v = bv;
        pv.i = pos;
        pv.j = bj;
    }
    return better;
}

// writes row `q` of the factored leading block: multipliers and remaining values of the table entry / correspondence row
template <int K>
__device__ __forceinline__ void leading_row(lds_double *T9, int q, uint32_t kind, double x, double y, double x_, double y_, uint32_t sig_lo,
                                            uint32_t sig_hi)
{
    double v[1][9];
    uint32_t pick_lo, pick_hi; // (kind and sigma are wave-uniform here)
    compose_pick((uint32_t)__builtin_amdgcn_readfirstlane((int)kind), sig_lo, sig_hi, &pick_lo, &pick_hi);
    row_pick(dlt_values(x, y, kind == 0 ? x_ : y_), pick_lo, pick_hi, v[0]);
    asm volatile("" ::: "memory");
    rows_eliminate<K, 1, false>(T9, v);
    if (threadIdx.x == 0)
    {
#pragma unroll
        for (int j = 0; j < 9; j++)
            T9[j * 9 + q] = v[0][j];
    }
}

template <int K>
__device__ __forceinline__ bool regen_lu_step(const regen_in &pd, uint32_t rows, lds_double *T9, lds_tab &tab, lu_state &st, uint32_t &sig_lo,
                                              uint32_t &sig_hi)
{
    const int lane = threadIdx.x;
    const uint32_t M = pd.M;
    __syncthreads(); // the table and the leading block of the previous step have landed
    sig_lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)sig_lo); // (wave-uniform by construction; the register indices want it in SGPRs)
    sig_hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)sig_hi);
    piv_t pv{-1.0, (uint32_t)K, (uint32_t)K};
    uint32_t cand = 0; // where the lane's best row came from: correspondence slot << 1 | a/b, or 0x80000000 | table entry
    uint32_t touched[K > 0 ? K : 1];
#pragma unroll
    for (int t = 0; t < K; t++)
        touched[t] = (uint32_t)__builtin_amdgcn_readfirstlane((int)tab.piv_match[t]);
    uint32_t pick_lo[3], pick_hi[3]; // position -> value index, per kind of row
#pragma unroll
    for (uint32_t kind = 0; kind < 3; kind++)
        compose_pick(kind, sig_lo, sig_hi, &pick_lo[kind], &pick_hi[kind]);
    // ---- the rows that never moved: a sweep over the correspondences, both rows of an inlier
    {
        // Two correspondences per lane and trip: four rows whose eliminations the scheduler interleaves (a row's steps are one
        // dependent chain of fp64 operations, and with two wavefronts on a SIMD there is little else to issue meanwhile).
        // The next trip's flags stay raw bytes until that trip (turned into predicates here they are waited for here, a
        // memory round trip per trip), and the loads take a clamped index instead of a branch around them (after a join
        // the compiler waits for every load).
        constexpr int SL = 2;
        uint32_t before = 0;
        uint32_t nflag[SL];
        double nx1[SL], ny1[SL], nx2[SL], ny2[SL];
#pragma unroll
        for (int q = 0; q < SL; q++)
        {
            const uint32_t c = min((uint32_t)(q * W + lane), M - 1);
            nflag[q] = pd.inl[c];
            nx1[q] = pd.x1[c], ny1[q] = pd.y1[c], nx2[q] = pd.x2[c], ny2[q] = pd.y2[c];
        }
        for (uint32_t base = 0; base < M; base += SL * W)
        {
            // (the U rows come from LDS in every trip: kept in registers across the loop they are up to 88 of them)
            asm volatile("" ::: "memory");
            bool take[SL];
            uint32_t rank[SL];
            double x1[SL], y1[SL], x2[SL], y2[SL];
#pragma unroll
            for (int q = 0; q < SL; q++)
            {
                const uint32_t i = base + q * W + lane;
                const bool f = i < M && nflag[q] != 0;
                x1[q] = nx1[q], y1[q] = ny1[q], x2[q] = nx2[q], y2[q] = ny2[q];
                const uint32_t nc = min(i + SL * W, M - 1);
                nflag[q] = pd.inl[nc];
                nx1[q] = pd.x1[nc], ny1[q] = pd.y1[nc], nx2[q] = pd.x2[nc], ny2[q] = pd.y2[nc];
                const unsigned long long mask = __ballot(f);
                rank[q] = before + __popcll(mask & ((1ull << lane) - 1ull));
                before += __popcll(mask);
                take[q] = f && rank[q] >= 5;
#pragma unroll
                for (int t = 0; t < K; t++)
                    take[q] = take[q] && i != touched[t];
            }
            if (take[0] || take[1])
            {
                double v[2 * SL][9];
                auto rows = [&]() {
#pragma unroll
                    for (int q = 0; q < SL; q++)
                    {
                        row_pick(dlt_values(x1[q], y1[q], x2[q]), pick_lo[0], pick_hi[0], v[2 * q]);
                        row_pick(dlt_values(x1[q], y1[q], y2[q]), pick_lo[1], pick_hi[1], v[2 * q + 1]);
                    }
                };
                rows();
                if (__ballot(rows_eliminate<K, 2 * SL, true>(T9, v)) != 0)
                {
#ifdef OCHIP_RANSAC_PHASES
                    if ((int)threadIdx.x == __builtin_ctzll(__ballot(true)))
                        atomicAdd(&g_phase[12], 1ull);
#endif
                    rows();
                    rows_eliminate<K, 2 * SL, false>(T9, v);
                }
#pragma unroll
                for (int q = 0; q < SL; q++)
                    if (take[q])
                    {
                        if (row_offer<K>(v[2 * q], 2 * rank[q], pv))
                            cand = (base / W + q) << 1;
                        if (row_offer<K>(v[2 * q + 1], 2 * rank[q] + 1, pv))
                            cand = (base / W + q) << 1 | 1u;
                    }
            }
        }
    }
    // ---- the rows of the table that are not pivots yet, one per lane
    double v_kk = 0.0; // (of the lane whose entry stands at position K: the value at (K, K))
    {
        // (the kind differs from lane to lane and the value picks are wave-uniform: a turn per kind, its lanes only)
        const bool mine = (uint32_t)lane < tab.n && !(tab.kind[lane] & 4u);
        const uint32_t kind = mine ? tab.kind[lane] : 3u;
        const double ex = mine ? tab.xy[lane][0] : 0.0, ey = mine ? tab.xy[lane][1] : 0.0;
        const double exp_ = mine ? (kind == 0 ? tab.xy[lane][2] : tab.xy[lane][3]) : 0.0;
        const uint32_t epos = mine ? tab.pos[lane] : 0u;
#pragma unroll
        for (uint32_t kd = 0; kd < 3; kd++)
            if (kind == kd)
            {
                double v[1][9];
                row_pick(dlt_values(ex, ey, exp_), pick_lo[kd], pick_hi[kd], v[0]);
                asm volatile("" ::: "memory");
                rows_eliminate<K, 1, false>(T9, v);
                v_kk = v[0][K];
                if (row_offer<K>(v[0], epos, pv))
                    cand = 0x80000000u | (uint32_t)lane;
            }
    }
    const double lv = pv.v;
    const uint32_t li = pv.i, lj = pv.j;
    piv_reduce(pv);
    double bv = pv.v;
    uint32_t bi = (uint32_t)__builtin_amdgcn_readfirstlane((int)pv.i), bj = (uint32_t)__builtin_amdgcn_readfirstlane((int)pv.j);
    const uint32_t at_k = (uint32_t)__builtin_amdgcn_readfirstlane((int)tab.top[K]);
    const double akk = bcast(v_kk, (int)at_k);
    uint32_t who; // the pivot row: cand of the lane that found it, or the entry at position K
    if (akk != akk) // a NaN in the first scanned cell sticks (nothing compares greater than NaN)
    {
        bv = akk;
        bi = K;
        bj = K;
        who = 0x80000000u | at_k;
    }
    else if (bv < 0) // every candidate was NaN: keep (k,k)
    {
        bv = fabs(akk);
        bi = K;
        bj = K;
        who = 0x80000000u | at_k;
    }
    else
    {
        const unsigned long long won = __ballot(lv == bv && li == bi && lj == bj);
        who = (uint32_t)__builtin_amdgcn_readlane((int)cand, __builtin_ctzll(won));
        if (!(who & 0x80000000u))
            who |= (uint32_t)__builtin_ctzll(won) << 24; // (a correspondence row: slot < 2^22, its lane beside it)
    }
    if (bv == 0.0)
        return false;
    if (bv > st.maxpivot)
        st.maxpivot = bv;
    st.rowT[K] = bi;
    st.colT[K] = bj;
    // ---- the pivot row: identity, then its multipliers and values into row K of the leading block (after the column
    //      transposition K <-> bj, which the rows above take too)
    uint32_t kind, entry = ~0u, match = ~0u;
    double x, y, x_, y_;
    if (who & 0x80000000u)
    {
        entry = who & 31u;
        kind = tab.kind[entry] & 3u;
        x = tab.xy[entry][0], y = tab.xy[entry][1], x_ = tab.xy[entry][2], y_ = tab.xy[entry][3];
    }
    else
    {
        match = ((who & 0x00FFFFFFu) >> 1) * W + (who >> 24);
        kind = who & 1u;
        x = pd.x1[match], y = pd.y1[match], x_ = pd.x2[match], y_ = pd.y2[match];
    }
    __syncthreads(); // every lane has read the U rows in the old arrangement
    if (bj != (uint32_t)K && lane < K)
    {
        const double t = T9[K * 9 + lane];
        T9[K * 9 + lane] = T9[bj * 9 + lane];
        T9[bj * 9 + lane] = t;
    }
    __syncthreads();
    if (bj != (uint32_t)K) // sigma: positions K and bj trade columns
    {
        unsigned long long sg = ((unsigned long long)sig_hi << 32) | sig_lo;
        const uint32_t a = nib_get(sg, K), b = nib_get(sg, bj);
        sg = nib_set(nib_set(sg, K, b), bj, a);
        sig_lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)sg);
        sig_hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(sg >> 32));
    }
    leading_row<K>(T9, K, kind, x, y, x_, y_, sig_lo, sig_hi); // (regenerated in the new arrangement: its value at position K is the pivot)
    // ---- the table: the pivot row goes to position K, the row that stood there to where the pivot row came from
    if (lane == 0)
    {
        uint32_t e = entry;
        if (e == ~0u)
        {
            e = tab.n;
            tab.xy[e][0] = x, tab.xy[e][1] = y, tab.xy[e][2] = x_, tab.xy[e][3] = y_;
            tab.xy[e + 1][0] = x, tab.xy[e + 1][1] = y, tab.xy[e + 1][2] = x_, tab.xy[e + 1][3] = y_;
            tab.kind[e + 1] = kind ^ 1u; // the sibling row stays where it is, but the sweep now skips its correspondence
            tab.pos[e + 1] = bi ^ 1u;
            tab.n = e + 2;
        }
        tab.piv_match[K] = match;
        tab.kind[e] = kind | 4u;
        tab.pos[e] = K;
        if (at_k != e)
        {
            tab.pos[at_k] = bi;
            if (bi < 9)
                tab.top[bi] = at_k;
        }
        tab.top[K] = e;
    }
    return true;
}

// (not inlined: the RANSAC kernels hold two models and a sample stream in registers around it, and with nine unrolled steps
// inside them the allocator gave up on two wavefronts per SIMD.  The pointers carry their address spaces across the call -
// generic ones would make every LDS access a flat one.)
__device__ __attribute__((noinline)) void regen_lu_solve9(regen_in pd, uint32_t n_in, lds_double *T9 /*LDS 81*/, lds_tab *tab_p, double *sol /*[9], uniform*/)
{
    lds_tab &tab = *tab_p;
    const int lane = threadIdx.x;
    const uint32_t M = pd.M, rows = 2 * n_in + 1;
    lu_state st;
    st.nonzero_pivots = 9;
    st.maxpivot = 0;
    __syncthreads();
    // the table starts with the rows of the first five inliers (rows 0 .. 9: the leading block and the row below it) and the last row
    {
        uint32_t before = 0;
        for (uint32_t base = 0; base < M && before < 5; base += W)
        {
            const uint32_t i = base + lane;
            const bool f = i < M && pd.inl[i];
            const unsigned long long mask = __ballot(f);
            const uint32_t rank = before + __popcll(mask & ((1ull << lane) - 1ull));
            before += __popcll(mask);
            if (f && rank < 5)
            {
                const double x = pd.x1[i], y = pd.y1[i], x_ = pd.x2[i], y_ = pd.y2[i];
                for (uint32_t ab = 0; ab < 2; ab++)
                {
                    const uint32_t e = 2 * rank + ab;
                    tab.xy[e][0] = x, tab.xy[e][1] = y, tab.xy[e][2] = x_, tab.xy[e][3] = y_;
                    tab.kind[e] = ab;
                    tab.pos[e] = e;
                }
            }
        }
        if (lane < 9)
        {
            tab.top[lane] = lane;
            tab.piv_match[lane] = ~0u;
        }
        if (lane == 0)
        {
            tab.xy[10][0] = tab.xy[10][1] = tab.xy[10][2] = tab.xy[10][3] = 0.0;
            tab.kind[10] = 2;
            tab.pos[10] = rows - 1;
            tab.n = 11;
        }
    }
    uint32_t sig_lo = 0x76543210u, sig_hi = 8u;
    int stop = 9;
    do
    {
#define OCHIP_LU_STEP(K)                                                                                               \
    if (!regen_lu_step<K>(pd, rows, T9, tab, st, sig_lo, sig_hi))                                                      \
    {                                                                                                                  \
        stop = K;                                                                                                      \
        break;                                                                                                         \
    }
        OCHIP_LU_STEP(0)
        OCHIP_LU_STEP(1)
        OCHIP_LU_STEP(2)
        OCHIP_LU_STEP(3)
        OCHIP_LU_STEP(4)
        OCHIP_LU_STEP(5)
        OCHIP_LU_STEP(6)
        OCHIP_LU_STEP(7)
        OCHIP_LU_STEP(8)
#undef OCHIP_LU_STEP
    } while (false);
    if (stop < 9)
    {
        // the remaining block is all zero: the rows standing at positions stop .. 8 close the leading block as they are
        st.nonzero_pivots = (uint32_t)stop;
        for (int i = stop; i < 9; i++)
        {
            st.rowT[i] = (uint32_t)i;
            st.colT[i] = (uint32_t)i;
        }
        __syncthreads();
        for (int q = stop; q < 9; q++)
        {
            const uint32_t e = tab.top[q];
            const uint32_t kind = tab.kind[e] & 3u;
            const double x = tab.xy[e][0], y = tab.xy[e][1], x_ = tab.xy[e][2], y_ = tab.xy[e][3];
            switch (stop)
            {
#define OCHIP_LEAD(K)                                                                                                  \
    case K: leading_row<K>(T9, q, kind, x, y, x_, y_, sig_lo, sig_hi); break;
                OCHIP_LEAD(0)
                OCHIP_LEAD(1)
                OCHIP_LEAD(2)
                OCHIP_LEAD(3)
                OCHIP_LEAD(4)
                OCHIP_LEAD(5)
                OCHIP_LEAD(6)
                OCHIP_LEAD(7)
                OCHIP_LEAD(8)
#undef OCHIP_LEAD
            }
        }
    }
    __syncthreads();
    lu_finish((const double *)T9, rows, 9, st, sol);
}

// the two DLT rows of one correspondence (homography_model.cpp:26-35), written column-major
__device__ __forceinline__ void write_dlt_rows(double *A, uint32_t ld, uint32_t r, double x, double y, double x_,
                                               double y_)
{
    const double a[9] = {-x, -y, -1, 0, 0, 0, x * x_, y * x_, x_};
    const double b[9] = {0, 0, 0, -x, -y, -1, x * y_, y * y_, y_};
    for (int j = 0; j < 9; j++)
    {
        A[(size_t)j * ld + r] = a[j];
        A[(size_t)j * ld + r + 1] = b[j];
    }
}

// homography_model::fitInliers (homography_model.cpp:52-87) on the flags pd.inl, of which n_in are set: the
// (2 n_in + 1) x 9 system in index order, its full-pivot LU, H from the solution.
__device__ __forceinline__ void fit_inliers(const pair_data &pd, uint32_t n_in, double *T9 /*LDS 81*/, tall_tab *tab /*LDS*/, model_t &model)
{
    const int lane = threadIdx.x;
    const uint32_t M = pd.M;
    double sol[9];
    const uint32_t rows = 2 * n_in + 1, ld = rows;
    if (rows > 9)
    {
        regen_in in;
        in.x1 = (glb_cdouble *)pd.x1, in.y1 = (glb_cdouble *)pd.y1, in.x2 = (glb_cdouble *)pd.x2, in.y2 = (glb_cdouble *)pd.y2;
        in.inl = (glb_cbyte *)pd.inl;
        in.M = pd.M;
        regen_lu_solve9(in, n_in, (lds_double *)T9, (lds_tab *)tab, sol);
        model_from_solution(model, sol);
        return;
    }
    // fewer than five inliers: the (2 n_in + 1) x 9 system in index order (homography_model.cpp:52-79), at most 9 x 9; the
    // small factorisation runs it from LDS
    uint32_t before = 0;
    bool nf = (uint32_t)lane < M && pd.inl[lane];
    double nx1 = nf ? pd.x1[lane] : 0.0, ny1 = nf ? pd.y1[lane] : 0.0, nx2 = nf ? pd.x2[lane] : 0.0,
           ny2 = nf ? pd.y2[lane] : 0.0;
    for (uint32_t base = 0; base < M; base += W)
    {
        const bool f = nf;
        const double x1 = nx1, y1 = ny1, x2 = nx2, y2 = ny2;
        {
            const uint32_t ni = base + W + lane;
            nf = ni < M && pd.inl[ni];
            nx1 = ni < M ? pd.x1[ni] : 0.0, ny1 = ni < M ? pd.y1[ni] : 0.0, nx2 = ni < M ? pd.x2[ni] : 0.0,
            ny2 = ni < M ? pd.y2[ni] : 0.0;
        }
        const unsigned long long mask = __ballot(f);
        if (f)
        {
            const uint32_t r = before + __popcll(mask & ((1ull << lane) - 1ull));
            write_dlt_rows(pd.P, ld, 2 * r, x1, y1, x2, y2);
        }
        before += __popcll(mask);
    }
    if (lane < 9)
        pd.P[(size_t)lane * ld + rows - 1] = lane == 8 ? 1.0 : 0.0;
    __syncthreads();
    for (uint32_t t = lane; t < rows * 9; t += W)
        T9[(t / rows) * 9 + (t % rows)] = pd.P[t];
    full_piv_lu_solve9(T9, rows, sol);
    model_from_solution(model, sol);
}

// checkSampleDegeneracy (homography_model.cpp:120-136) on measurement1.hnormalized(): any three of the four points within
// 1e-10 of a line
__device__ __forceinline__ bool sample_degenerate(const double (&px)[4], const double (&py)[4])
{
    bool degenerate = false;
    for (int a = 0; a < 4; a++)
        for (int b = a + 1; b < 4; b++)
            for (int c = b + 1; c < 4; c++)
            {
                const double v1x = px[b] - px[a], v1y = py[b] - py[a];
                const double v2x = px[c] - px[a], v2y = py[c] - py[a];
                if (fabs(v1x * v2y - v1y * v2x) < 1e-10)
                    degenerate = true;
            }
    return degenerate;
}

// homography_model::fit of one lane's sample; element (i, j) of the lane's 9 x 9 system lives at Aq[(j * 9 + i) * FB]
// (ransac_epipolar.hip has no use for it)
[[maybe_unused]] __device__ void lane_fit(double *Aq /*already offset by the lane*/, const double *px, const double *py, const double *qx,
                         const double *qy, model_t &m)
{
#define AQ(i, j) Aq[(((j) * 9 + (i)) * FB)]
#pragma unroll
    for (int t = 0; t < 81; t++)
        Aq[t * FB] = 0.0;
#pragma unroll
    for (int p = 0; p < 4; p++)
    {
        const double x = px[p], y = py[p], x_ = qx[p], y_ = qy[p];
        AQ(2 * p, 0) = -x;
        AQ(2 * p, 1) = -y;
        AQ(2 * p, 2) = -1;
        AQ(2 * p, 6) = x * x_;
        AQ(2 * p, 7) = y * x_;
        AQ(2 * p, 8) = x_;
        AQ(2 * p + 1, 3) = -x;
        AQ(2 * p + 1, 4) = -y;
        AQ(2 * p + 1, 5) = -1;
        AQ(2 * p + 1, 6) = x * y_;
        AQ(2 * p + 1, 7) = y * y_;
        AQ(2 * p + 1, 8) = y_;
    }
    AQ(8, 8) = 1.0;

    uint64_t rowT = 0x876543210ull, colT = 0x876543210ull;
    uint32_t nonzero_pivots = 9;
    double maxpivot = 0;
    bool alive = true;
#pragma unroll
    for (int k = 0; k < 9; k++)
    {
        if (alive)
        {
            double bv = -1.0;
            uint32_t bi = k, bj = k;
#pragma unroll
            for (int j = k; j < 9; j++)
#pragma unroll
                for (int i = k; i < 9; i++)
                {
                    const double v = fabs(AQ(i, j));
                    if (v > bv) // column-by-column scan, strict '>' keeps the first maximum
                    {
                        bv = v;
                        bi = i;
                        bj = j;
                    }
                }
            const double akk = AQ(k, k);
            if (akk != akk)
            {
                bv = akk;
                bi = k;
                bj = k;
            }
            else if (bv < 0)
            {
                bv = fabs(akk);
                bi = k;
                bj = k;
            }
            if (bv == 0.0)
            {
                nonzero_pivots = k;
                alive = false; // the remaining transpositions stay the identity
            }
            else
            {
                if (bv > maxpivot)
                    maxpivot = bv;
                rowT = nib_set(rowT, k, bi);
                colT = nib_set(colT, k, bj);
                if ((uint32_t)k != bi)
                {
#pragma unroll
                    for (int j = 0; j < 9; j++)
                    {
                        const double t = AQ(k, j);
                        AQ(k, j) = AQ(bi, j);
                        AQ(bi, j) = t;
                    }
                }
                if ((uint32_t)k != bj)
                {
#pragma unroll
                    for (int i = 0; i < 9; i++)
                    {
                        const double t = AQ(i, k);
                        AQ(i, k) = AQ(i, bj);
                        AQ(i, bj) = t;
                    }
                }
                const double p = AQ(k, k);
                double rowk[9];
#pragma unroll
                for (int j = k + 1; j < 9; j++)
                    rowk[j] = AQ(k, j);
#pragma unroll
                for (int i = k + 1; i < 9; i++)
                {
                    const double l = AQ(i, k) / p;
                    AQ(i, k) = l;
#pragma unroll
                    for (int j = k + 1; j < 9; j++)
                        AQ(i, j) = AQ(i, j) - l * rowk[j];
                }
            }
        }
    }
    // rank, P e_last, the two substitutions, the column permutation (lu_finish, per lane)
    const double premult = fabs(maxpivot) * (2.220446049250313e-16 * (double)9);
    uint32_t rank = 0;
#pragma unroll
    for (int i = 0; i < 9; i++)
        if ((uint32_t)i < nonzero_pivots)
            rank += (fabs(AQ(i, i)) > premult) ? 1 : 0;
    double sol[9];
#pragma unroll
    for (int i = 0; i < 9; i++)
        sol[i] = 0;
    if (rank != 0)
    {
        uint32_t pos = 8;
#pragma unroll
        for (int k = 0; k < 9; k++)
        {
            const uint32_t r = nib_get(rowT, k);
            if (pos == (uint32_t)k)
                pos = r;
            else if (pos == r)
                pos = k;
        }
        double c[9];
#pragma unroll
        for (int i = 0; i < 9; i++)
            c[i] = ((uint32_t)i == pos) ? 1.0 : 0.0;
#pragma unroll
        for (int j = 0; j < 9; j++)
        {
            const double cj = c[j];
#pragma unroll
            for (int i = j + 1; i < 9; i++)
                c[i] -= cj * AQ(i, j);
        }
#pragma unroll
        for (int jj = 8; jj >= 0; jj--)
            if ((uint32_t)jj < rank)
            {
                c[jj] /= AQ(jj, jj);
                const double cj = c[jj];
#pragma unroll
                for (int i = 0; i < jj; i++)
                    c[i] -= cj * AQ(i, jj);
            }
        uint64_t perm = 0x876543210ull;
#pragma unroll
        for (int k = 0; k < 9; k++)
        {
            const uint32_t ck = nib_get(colT, k);
            const uint32_t t = nib_get(perm, k);
            perm = nib_set(perm, k, nib_get(perm, ck));
            perm = nib_set(perm, ck, t);
        }
#pragma unroll
        for (int i = 0; i < 9; i++)
            if ((uint32_t)i < rank)
            {
                const uint32_t pi = nib_get(perm, i);
#pragma unroll
                for (int mm = 0; mm < 9; mm++)
                    if (pi == (uint32_t)mm)
                        sol[mm] = c[i];
            }
    }
#undef AQ
    model_from_solution(m, sol);
}

// the scoring walk's error of a homography (ransac_loop.hpp: score_walk)
__device__ __forceinline__ double model_error(const model_t &m, double x1, double y1, double x2, double y2)
{
    return transfer_error(m, x1, y1, x2, y2);
}

} // namespace
