// car_pose.hip — relative pose of an unposed pair from keypoint matches (include/car_hip.h: car_essential_*).
//
// The reference calls cv2.findEssentialMat(RANSAC) + cv2.recoverPose (dataset/load_video_superglue.py:114-138).  Here a fixed budget of
// H five-point hypotheses is solved and scored exhaustively on the device, all in fp64; recoverPose stays on the host (harness.py).
//
// essential_solve_kernel: one lane per hypothesis, 64 hypotheses per workgroup, each with 200 doubles of LDS (element i of lane l at
// lds[i * 64 + l]: every runtime-indexed array of the solver lives there, none in scratch).  Nistér's formulation:
//   1. the 5 x 9 epipolar system, Gauss-Jordan with complete pivoting -> the null space X, Y, Z, W; E = x X + y Y + z Z + W
//   2. the ten cubics (E E^T - tr(E E^T) / 2) E = 0 and det E = 0 as a 10 x 20 matrix in Nistér's monomial order, built in registers with
//      compile-time indices, rows scaled to unit maximum, Gauss-Jordan with partial pivoting on the first ten columns
//   3. rows <x^2 z> - z <x^2>, <y^2 z> - z <y^2>, <xyz> - z <xy> form B(z) (x, y, 1)^T = 0; det B(z) is the degree-10 polynomial
//   4. its real roots through the chain of derivatives: the roots of p^(k+1) split the line into intervals on which p^(k) is
//      monotone, a sign change in one is bisected (at most 128 halvings, which resolve a root to 2^-57 because a hypothesis whose root
//      bound exceeds 2^70 is refused).  Every loop has a fixed bound; nothing runs "until converged".
//   5. per root: x, y from the pair of rows of B(z) whose cross product has the largest last component; three Gauss-Newton steps on the
//      ten constraints themselves in (x, y, z), each kept only if it lowers their norm (an elimination with a small pivot leaves roots
//      good to 1e-6 only; the constraints do not pass through it); E scaled to unit norm.
// essential_score_kernel: 32 hypotheses x 10 candidates per workgroup, the matches staged through LDS 512 at a time and read as
// broadcasts; counts the Sampson errors below thresh^2 (a NaN compares false: no inlier).
// essential_select_kernel: one workgroup.  The winner is the maximum of (count << 32 | ~slot), slot = 10 hypothesis + candidate: the
// largest count, then the lowest hypothesis, then the lowest candidate, whatever the schedule.  Integer maxima only, no float atomics.
//
// essential_solve_one is __host__ __device__, so the same text runs on the host for debugging.
#include "car_common.h"
#include <math.h>

namespace {

constexpr int kSolveLanes = 64;                  // hypotheses per workgroup of the solver
constexpr int kSolveSlots = 200;                 // doubles of LDS per hypothesis (the 10 x 20 matrix is the largest tenant)
constexpr int kCands = 10;
constexpr int kScoreHyp = 32, kScoreThreads = kScoreHyp * kCands, kChunk = 512;
constexpr int kSelectThreads = 1024;
constexpr int kMaxN = 1 << 24, kMaxH = 1 << 24;  // 10 H slots and N matches stay far inside 32-bit indices
constexpr double kPivotEps = 1e-13;              // a pivot at or below this share of its matrix's scale counts as zero
constexpr int kBisect = 128;
constexpr double kMaxBound = 0x1p70;             // the largest root bound kBisect halvings resolve to a double's precision near 1

struct Mem {                                     // a hypothesis's private array: element i
    double* p;
    int stride;
    __host__ __device__ double& operator()(int i) const { return p[(size_t)i * stride]; }
};

// monomial slots: linear x y z 1; quadratic xx xy xz yy yz zz x y z 1; cubic in Nistér's column order
// x3 y3 x2y xy2 x2z x2 y2z y2 xyz xy | xz2 xz x yz2 yz y z3 z2 z 1
__host__ __device__ constexpr int q2(int a, int b) {
    const int t[16] = {0, 1, 2, 6, 1, 3, 4, 7, 2, 4, 5, 8, 6, 7, 8, 9};
    return t[a * 4 + b];
}
__host__ __device__ constexpr int c3(int q, int l) {
    const int t[40] = {0, 2, 4, 5, 2, 3, 8, 9, 4, 8, 10, 11, 3, 1, 6, 7, 8, 6, 13, 14, 10, 13, 16, 17, 5, 9, 11, 12, 9, 7, 14, 15,
                       11, 14, 17, 18, 12, 15, 18, 19};
    return t[q * 4 + l];
}
__host__ __device__ constexpr int sym(int i, int j) {          // slot of the symmetric 3 x 3 entry (i, j)
    const int t[9] = {0, 1, 2, 1, 3, 4, 2, 4, 5};
    return t[i * 3 + j];
}

// level d (a polynomial of degree d, d = 1..10) of the derivative chain starts at element d (d + 1) / 2 - 1: 65 doubles in all
__host__ __device__ inline int level_at(int d) { return d * (d + 1) / 2 - 1; }
constexpr int kPrev = 65, kCur = 75, kB = 85;                   // roots of the level below / this level; B(z): 3 rows of 4 + 4 + 5

__host__ __device__ inline double chain_eval(const Mem& m, int d, double z) {
    const int at = level_at(d);
    double v = m(at + d);
    for (int i = d - 1; i >= 0; --i) v = v * z + m(at + i);
    return v;
}

// ---- root polishing: Gauss-Newton on the ten constraints themselves, f(E) = (2 E E^T E - tr(E E^T) E, det E), in the unknowns (x, y, z)
// of E = x X + y Y + z Z + W.  3 x 3 matrices are row-major double[9]; every index is a compile-time constant.
__host__ __device__ inline void mat_mul(const double* a, const double* b, double* c) {          // c = a b
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) c[3 * i + j] = a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j] + a[3 * i + 2] * b[6 + j];
}
__host__ __device__ inline void mat_mul_nt(const double* a, const double* b, double* c) {       // c = a b^T
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) c[3 * i + j] = a[3 * i] * b[3 * j] + a[3 * i + 1] * b[3 * j + 1] + a[3 * i + 2] * b[3 * j + 2];
}
__host__ __device__ inline void mat_mul_tn(const double* a, const double* b, double* c) {       // c = a^T b
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) c[3 * i + j] = a[i] * b[j] + a[3 + i] * b[3 + j] + a[6 + i] * b[6 + j];
}
__host__ __device__ inline void cofactors(const double* e, double* c) {
    c[0] = e[4] * e[8] - e[5] * e[7]; c[1] = e[5] * e[6] - e[3] * e[8]; c[2] = e[3] * e[7] - e[4] * e[6];
    c[3] = e[2] * e[7] - e[1] * e[8]; c[4] = e[0] * e[8] - e[2] * e[6]; c[5] = e[1] * e[6] - e[0] * e[7];
    c[6] = e[1] * e[5] - e[2] * e[4]; c[7] = e[2] * e[3] - e[0] * e[5]; c[8] = e[0] * e[4] - e[1] * e[3];
}
// f [10] at E; G = E E^T and its trace are returned for the derivative.  Returns |f|^2.
__host__ __device__ inline double constraints_at(const double* E, double* f, double* G, double* tr) {
    mat_mul_nt(E, E, G);
    *tr = G[0] + G[4] + G[8];
    double GE[9], ss = 0.0;
    mat_mul(G, E, GE);
#pragma unroll
    for (int i = 0; i < 9; ++i) f[i] = 2.0 * GE[i] - *tr * E[i];
    f[9] = E[0] * (E[4] * E[8] - E[5] * E[7]) - E[1] * (E[3] * E[8] - E[5] * E[6]) + E[2] * (E[3] * E[7] - E[4] * E[6]);
#pragma unroll
    for (int i = 0; i < 10; ++i) ss += f[i] * f[i];
    return ss;
}
// the derivative of f along D: 2 (D E^T E + E D^T E + E E^T D) - 2 tr(E D^T) E - tr(E E^T) D, and sum(cof(E) D)
__host__ __device__ inline void constraints_along(const double* E, const double* G, double tr, const double* cof, const double* D, double* df) {
    double S[9], SE[9], StE[9], GD[9];
    mat_mul_nt(D, E, S);
    mat_mul(S, E, SE);
    mat_mul_tn(S, E, StE);
    mat_mul(G, D, GD);
    const double trS = S[0] + S[4] + S[8];
    double dd = 0.0;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        df[i] = 2.0 * (SE[i] + StE[i] + GD[i]) - 2.0 * trS * E[i] - tr * D[i];
        dd += cof[i] * D[i];
    }
    df[9] = dd;
}
constexpr int kPolish = 3;
// (x, y, z) -> the polished unknowns; a step is kept only when it lowers |f|^2
__host__ __device__ inline void polish_root(const double X[4][9], double* u) {
    double E[9], f[10], G[9], tr;
#pragma unroll
    for (int e = 0; e < 9; ++e) E[e] = u[0] * X[0][e] + u[1] * X[1][e] + u[2] * X[2][e] + X[3][e];
    double ss = constraints_at(E, f, G, &tr);
    for (int it = 0; it < kPolish; ++it) {
        double cof[9], J[3][10];
        cofactors(E, cof);
#pragma unroll
        for (int d = 0; d < 3; ++d) constraints_along(E, G, tr, cof, X[d], J[d]);
        double A[6] = {0, 0, 0, 0, 0, 0}, b[3] = {0, 0, 0};                                  // J^T J (00 01 02 11 12 22), -J^T f
#pragma unroll
        for (int i = 0; i < 10; ++i) {
            A[0] += J[0][i] * J[0][i]; A[1] += J[0][i] * J[1][i]; A[2] += J[0][i] * J[2][i];
            A[3] += J[1][i] * J[1][i]; A[4] += J[1][i] * J[2][i]; A[5] += J[2][i] * J[2][i];
            b[0] -= J[0][i] * f[i]; b[1] -= J[1][i] * f[i]; b[2] -= J[2][i] * f[i];
        }
        const double c00 = A[3] * A[5] - A[4] * A[4], c01 = A[2] * A[4] - A[1] * A[5], c02 = A[1] * A[4] - A[2] * A[3];
        const double c11 = A[0] * A[5] - A[2] * A[2], c12 = A[1] * A[2] - A[0] * A[4], c22 = A[0] * A[3] - A[1] * A[1];
        const double det = A[0] * c00 + A[1] * c01 + A[2] * c02;
        const double v[3] = {u[0] + (c00 * b[0] + c01 * b[1] + c02 * b[2]) / det, u[1] + (c01 * b[0] + c11 * b[1] + c12 * b[2]) / det,
                             u[2] + (c02 * b[0] + c12 * b[1] + c22 * b[2]) / det};
        double E2[9], f2[10], G2[9], tr2;
#pragma unroll
        for (int e = 0; e < 9; ++e) E2[e] = v[0] * X[0][e] + v[1] * X[1][e] + v[2] * X[2][e] + X[3][e];
        const double ss2 = constraints_at(E2, f2, G2, &tr2);
        if (!(ss2 < ss)) break;                                                              // also a NaN: the step is dropped
        ss = ss2;
        tr = tr2;
#pragma unroll
        for (int e = 0; e < 9; ++e) { E[e] = E2[e]; G[e] = G2[e]; }
#pragma unroll
        for (int i = 0; i < 10; ++i) f[i] = f2[i];
        u[0] = v[0]; u[1] = v[1]; u[2] = v[2];
    }
}

// Returns the number of candidates written to cand[10][9] (zeroed by the caller); 0 for a refused hypothesis.
__host__ __device__ inline int essential_solve_one(const double* __restrict__ x0, const double* __restrict__ x1, int N,
                                                   const int* __restrict__ s, const Mem m, double* __restrict__ cand) {
    int idx[5];
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        idx[k] = s[k];
        ok = ok && idx[k] >= 0 && idx[k] < N;
    }
#pragma unroll
    for (int k = 1; k < 5; ++k)
#pragma unroll
        for (int j = 0; j < k; ++j) ok = ok && idx[k] != idx[j];
    if (!ok) return 0;                                          // nothing was read through a bad index

    // ---- 1. x1^T E x0 = 0, E row-major: A [5][9] at m(9 r + c)
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const double h0[3] = {x0[2 * (size_t)idx[k]], x0[2 * (size_t)idx[k] + 1], 1.0};
        const double h1[3] = {x1[2 * (size_t)idx[k]], x1[2 * (size_t)idx[k] + 1], 1.0};
        ok = ok && __builtin_isfinite(h0[0]) && __builtin_isfinite(h0[1]) && __builtin_isfinite(h1[0]) && __builtin_isfinite(h1[1]);
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) m(k * 9 + 3 * r + c) = h1[r] * h0[c];
    }
    if (!ok) return 0;
    double scale = 0.0;
    for (int i = 0; i < 45; ++i) scale = fmax(scale, fabs(m(i)));
    if (!__builtin_isfinite(scale)) return 0;                   // a product overflowed

    unsigned long long perm = 0x876543210ULL;                   // nibble j: the original column now at position j
    for (int k = 0; k < 5; ++k) {
        double best = -1.0;
        int pr = k, pc = k;
        for (int r = k; r < 5; ++r)
            for (int c = k; c < 9; ++c) {
                const double v = fabs(m(r * 9 + c));
                if (v > best) { best = v; pr = r; pc = c; }     // first maximum in row-major order; a NaN never wins
            }
        if (!(best > kPivotEps * scale)) return 0;
        if (pr != k)
            for (int c = 0; c < 9; ++c) { const double t = m(k * 9 + c); m(k * 9 + c) = m(pr * 9 + c); m(pr * 9 + c) = t; }
        if (pc != k) {
            for (int r = 0; r < 5; ++r) { const double t = m(r * 9 + k); m(r * 9 + k) = m(r * 9 + pc); m(r * 9 + pc) = t; }
            const unsigned long long a = (perm >> (4 * k)) & 15, b = (perm >> (4 * pc)) & 15;
            perm = (perm & ~((15ULL << (4 * k)) | (15ULL << (4 * pc)))) | (b << (4 * k)) | (a << (4 * pc));
        }
        const double piv = m(k * 9 + k);
        for (int c = 0; c < 9; ++c) m(k * 9 + c) = m(k * 9 + c) / piv;
        for (int r = 0; r < 5; ++r) {
            if (r == k) continue;
            const double f = m(r * 9 + k);
            for (int c = 0; c < 9; ++c) m(r * 9 + c) = m(r * 9 + c) - f * m(k * 9 + c);
        }
    }
    // null vector f in permuted coordinates: (-A[:, 5 + f], e_f); scattered to the original columns at m(45 + 9 f + column)
    for (int f = 0; f < 4; ++f)
        for (int j = 0; j < 9; ++j) {
            const double v = j < 5 ? -m(j * 9 + 5 + f) : (j == 5 + f ? 1.0 : 0.0);
            m(45 + 9 * f + (int)((perm >> (4 * j)) & 15)) = v;
        }
    double X[4][9];                                             // compile-time indices from here on: registers
#pragma unroll
    for (int f = 0; f < 4; ++f)
#pragma unroll
        for (int e = 0; e < 9; ++e) X[f][e] = m(45 + 9 * f + e);

    // ---- 2. the ten cubics.  L = E E^T - tr(E E^T) / 2 (symmetric, quadratic entries), rows 0-8 = L E, row 9 = det E
    {
        double L[6][10];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = i; j < 3; ++j) {
                double q[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
                for (int k = 0; k < 3; ++k)
#pragma unroll
                    for (int a = 0; a < 4; ++a)
#pragma unroll
                        for (int b = 0; b < 4; ++b) q[q2(a, b)] += X[a][3 * i + k] * X[b][3 * j + k];
#pragma unroll
                for (int t = 0; t < 10; ++t) L[sym(i, j)][t] = q[t];
            }
#pragma unroll
        for (int t = 0; t < 10; ++t) {
            const double half_tr = 0.5 * (L[0][t] + L[3][t] + L[5][t]);
            L[0][t] -= half_tr;
            L[3][t] -= half_tr;
            L[5][t] -= half_tr;
        }
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                double row[20] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
                for (int k = 0; k < 3; ++k)
#pragma unroll
                    for (int q = 0; q < 10; ++q)
#pragma unroll
                        for (int l = 0; l < 4; ++l) row[c3(q, l)] += L[sym(i, k)][q] * X[l][3 * k + j];
                double mx = 0.0;
#pragma unroll
                for (int t = 0; t < 20; ++t) mx = fmax(mx, fabs(row[t]));
                if (!(mx > 0.0) || !__builtin_isfinite(mx)) ok = false;
#pragma unroll
                for (int t = 0; t < 20; ++t) m((3 * i + j) * 20 + t) = row[t] / mx;
            }
    }
    {
        // det E = E00 (E11 E22 - E12 E21) - E01 (E10 E22 - E12 E20) + E02 (E10 E21 - E11 E20)
        double row[20] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int c1 = c == 0 ? 1 : 0, c2 = c == 2 ? 1 : 2;                 // the minor's columns, ascending
            const double sgn = c == 1 ? -1.0 : 1.0;
            double q[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) q[q2(a, b)] += X[a][3 + c1] * X[b][6 + c2] - X[a][3 + c2] * X[b][6 + c1];
#pragma unroll
            for (int t = 0; t < 10; ++t)
#pragma unroll
                for (int l = 0; l < 4; ++l) row[c3(t, l)] += sgn * q[t] * X[l][c];
        }
        double mx = 0.0;
#pragma unroll
        for (int t = 0; t < 20; ++t) mx = fmax(mx, fabs(row[t]));
        if (!(mx > 0.0) || !__builtin_isfinite(mx)) ok = false;
#pragma unroll
        for (int t = 0; t < 20; ++t) m(9 * 20 + t) = row[t] / mx;
    }
    if (!ok) return 0;

    for (int k = 0; k < 10; ++k) {
        double best = -1.0;
        int pr = k;
        for (int r = k; r < 10; ++r) {
            const double v = fabs(m(r * 20 + k));
            if (v > best) { best = v; pr = r; }
        }
        if (!(best > kPivotEps)) return 0;
        if (pr != k)
            for (int c = k; c < 20; ++c) { const double t = m(k * 20 + c); m(k * 20 + c) = m(pr * 20 + c); m(pr * 20 + c) = t; }
        const double piv = m(k * 20 + k);
        for (int c = k; c < 20; ++c) m(k * 20 + c) = m(k * 20 + c) / piv;
        for (int r = 0; r < 10; ++r) {
            if (r == k) continue;
            const double f = m(r * 20 + k);
            for (int c = k; c < 20; ++c) m(r * 20 + c) = m(r * 20 + c) - f * m(k * 20 + c);
        }
    }

    // ---- 3. B(z), coefficients ascending: row g of (bx[4], by[4], bc[5]); then p = det B
    double B[3][13];
#pragma unroll
    for (int g = 0; g < 3; ++g) {
        double a[10], b[10];
#pragma unroll
        for (int t = 0; t < 10; ++t) {
            a[t] = m((4 + 2 * g) * 20 + 10 + t);
            b[t] = m((5 + 2 * g) * 20 + 10 + t);
        }
        B[g][0] = a[2]; B[g][1] = a[1] - b[2]; B[g][2] = a[0] - b[1]; B[g][3] = -b[0];
        B[g][4] = a[5]; B[g][5] = a[4] - b[5]; B[g][6] = a[3] - b[4]; B[g][7] = -b[3];
        B[g][8] = a[9]; B[g][9] = a[8] - b[9]; B[g][10] = a[7] - b[8]; B[g][11] = a[6] - b[7]; B[g][12] = -b[6];
    }
    double p[11] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int g = 0; g < 3; ++g) {
        // expansion along the first row of columns: bx_0 (by_1 bc_2 - by_2 bc_1) - bx_1 (by_0 bc_2 - by_2 bc_0) + bx_2 (by_0 bc_1 - by_1 bc_0)
        const int r1 = g == 0 ? 1 : 0, r2 = g == 2 ? 1 : 2;
        const double sgn = g == 1 ? -1.0 : 1.0;
        double minor[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 5; ++j) minor[i + j] += B[r1][4 + i] * B[r2][8 + j] - B[r2][4 + i] * B[r1][8 + j];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 8; ++j) p[i + j] += sgn * B[g][i] * minor[j];
    }
    double pmax = 0.0;
#pragma unroll
    for (int t = 0; t < 11; ++t) pmax = fmax(pmax, fabs(p[t]));
    if (!(pmax > 0.0) || !__builtin_isfinite(pmax)) return 0;
    double low = 0.0;
#pragma unroll
    for (int t = 0; t < 11; ++t) {
        p[t] = p[t] / pmax;
        if (t < 10) low = fmax(low, fabs(p[t]));
    }
    // Cauchy: every root lies inside (-bound, bound).  kBisect halvings of an interval of 2 bound leave 2^-57 of absolute width when
    // bound < 2^70, below the spacing of doubles near 1; a leading coefficient so small that the bound is larger refuses the hypothesis
    const double bound = 1.0 + low / fabs(p[10]);
    if (!__builtin_isfinite(1.0 / p[10]) || !(bound < kMaxBound)) return 0;

    // the matrix is spent: its LDS now holds the derivative chain, the roots and B(z)
#pragma unroll
    for (int g = 0; g < 3; ++g)
#pragma unroll
        for (int t = 0; t < 13; ++t) m(kB + 13 * g + t) = B[g][t];
#pragma unroll
    for (int t = 0; t < 11; ++t) m(level_at(10) + t) = p[t];
    for (int d = 10; d >= 2; --d)
        for (int i = 0; i < d; ++i) m(level_at(d - 1) + i) = (double)(i + 1) * m(level_at(d) + i + 1);

    // ---- 4. real roots, ascending
    int nprev = 0;
    for (int d = 1; d <= 10; ++d) {
        int ncur = 0;
        double lo = -bound, flo = chain_eval(m, d, lo);
        for (int j = 0; j <= nprev; ++j) {
            const double hi = j < nprev ? m(kPrev + j) : bound;
            const double fhi = chain_eval(m, d, hi);
            if ((flo < 0.0) != (fhi < 0.0) && ncur < d) {
                double a = lo, b = hi;
                const bool neg = flo < 0.0;
                for (int it = 0; it < kBisect; ++it) {
                    const double mid = a + 0.5 * (b - a);
                    if (!(mid > a && mid < b)) break;
                    if ((chain_eval(m, d, mid) < 0.0) == neg) a = mid; else b = mid;
                }
                m(kCur + ncur) = a + 0.5 * (b - a);
                ++ncur;
            }
            lo = hi;
            flo = fhi;
        }
        for (int j = 0; j < ncur; ++j) m(kPrev + j) = m(kCur + j);
        nprev = ncur;
    }

    // ---- 5. candidates
    int n = 0;
    for (int j = 0; j < nprev; ++j) {
        const double z = m(kPrev + j);
        double rows[3][3];
#pragma unroll
        for (int g = 0; g < 3; ++g) {
            const int at = kB + 13 * g;
            rows[g][0] = ((m(at + 3) * z + m(at + 2)) * z + m(at + 1)) * z + m(at + 0);
            rows[g][1] = ((m(at + 7) * z + m(at + 6)) * z + m(at + 5)) * z + m(at + 4);
            rows[g][2] = (((m(at + 12) * z + m(at + 11)) * z + m(at + 10)) * z + m(at + 9)) * z + m(at + 8);
        }
        double cx = 0.0, cy = 0.0, cw = 0.0, best = -1.0;
#pragma unroll
        for (int pair = 0; pair < 3; ++pair) {
            const int ra = pair == 2 ? 1 : 0, rb = pair == 0 ? 1 : 2;          // (0,1) (0,2) (1,2)
            const double vx = rows[ra][1] * rows[rb][2] - rows[ra][2] * rows[rb][1];
            const double vy = rows[ra][2] * rows[rb][0] - rows[ra][0] * rows[rb][2];
            const double vw = rows[ra][0] * rows[rb][1] - rows[ra][1] * rows[rb][0];
            if (fabs(vw) > best) { best = fabs(vw); cx = vx; cy = vy; cw = vw; }
        }
        double u[3] = {cx / cw, cy / cw, z};
        if (__builtin_isfinite(u[0]) && __builtin_isfinite(u[1])) polish_root(X, u);
        double E[9], ss = 0.0;
#pragma unroll
        for (int e = 0; e < 9; ++e) {
            E[e] = u[0] * X[0][e] + u[1] * X[1][e] + u[2] * X[2][e] + X[3][e];
            ss += E[e] * E[e];
        }
        const double nrm = sqrt(ss);
        bool fin = nrm > 0.0 && __builtin_isfinite(nrm);
#pragma unroll
        for (int e = 0; e < 9; ++e) {
            E[e] = E[e] / nrm;
            fin = fin && __builtin_isfinite(E[e]);
        }
        if (!fin || n >= kCands) continue;
#pragma unroll
        for (int e = 0; e < 9; ++e) cand[n * 9 + e] = E[e];
        ++n;
    }
    return n;
}

__global__ __launch_bounds__(kSolveLanes) void essential_solve_kernel(const double* __restrict__ x0, const double* __restrict__ x1, int N,
                                                                      const int* __restrict__ samples, int H, double* __restrict__ cand,
                                                                      int* __restrict__ nsol) {
    extern __shared__ double solve_lds[];
    const int h = blockIdx.x * kSolveLanes + threadIdx.x;
    if (h >= H) return;                                         // the kernel has no barrier
    double* out = cand + (size_t)h * (kCands * 9);
    for (int i = 0; i < kCands * 9; ++i) out[i] = 0.0;
    nsol[h] = essential_solve_one(x0, x1, N, samples + (size_t)h * 5, Mem{solve_lds + threadIdx.x, kSolveLanes}, out);
}

// cv2's error for the model; match = (x, y) in the first view, (u, v) in the second
__device__ __forceinline__ bool sampson_inlier(const double* e, double x, double y, double u, double v, double thr2) {
    const double a = e[0] * x + e[1] * y + e[2];
    const double b = e[3] * x + e[4] * y + e[5];
    const double c = e[6] * x + e[7] * y + e[8];
    const double ta = e[0] * u + e[3] * v + e[6];
    const double tb = e[1] * u + e[4] * v + e[7];
    const double r = u * a + v * b + c;
    return (r * r) / (a * a + b * b + ta * ta + tb * tb) < thr2;               // false for a NaN
}

__global__ __launch_bounds__(kScoreThreads) void essential_score_kernel(const double* __restrict__ x0, const double* __restrict__ x1, int N,
                                                                        const double* __restrict__ cand, const int* __restrict__ nsol, int H,
                                                                        double thr2, int* __restrict__ counts, int* __restrict__ hyp_best) {
    __shared__ double sm[kChunk * 4];
    __shared__ int cnt[kScoreThreads];
    const int tid = threadIdx.x;
    const int h = blockIdx.x * kScoreHyp + tid / kCands, c = tid % kCands;
    const bool live = h < H && c < nsol[h < H ? h : 0];
    double e[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) e[i] = live ? cand[((size_t)h * kCands + c) * 9 + i] : 0.0;
    int count = 0;
    for (int base = 0; base < N; base += kChunk) {
        const int n = N - base < kChunk ? N - base : kChunk;
        for (int i = tid; i < n; i += kScoreThreads) {
            sm[4 * i + 0] = x0[2 * (size_t)(base + i)];
            sm[4 * i + 1] = x0[2 * (size_t)(base + i) + 1];
            sm[4 * i + 2] = x1[2 * (size_t)(base + i)];
            sm[4 * i + 3] = x1[2 * (size_t)(base + i) + 1];
        }
        __syncthreads();
        if (live)
            for (int i = 0; i < n; ++i) count += sampson_inlier(e, sm[4 * i], sm[4 * i + 1], sm[4 * i + 2], sm[4 * i + 3], thr2) ? 1 : 0;
        __syncthreads();
    }
    if (h < H) counts[(size_t)h * kCands + c] = count;
    cnt[tid] = count;
    __syncthreads();
    if (tid < kScoreHyp && blockIdx.x * kScoreHyp + tid < H) {
        int best = 0;
        for (int k = 0; k < kCands; ++k) best = cnt[tid * kCands + k] > best ? cnt[tid * kCands + k] : best;
        hyp_best[blockIdx.x * kScoreHyp + tid] = best;
    }
}

__global__ __launch_bounds__(kSelectThreads) void essential_select_kernel(const double* __restrict__ x0, const double* __restrict__ x1, int N,
                                                                          const double* __restrict__ cand, const int* __restrict__ nsol,
                                                                          const int* __restrict__ counts, int H, double thr2,
                                                                          double* __restrict__ E, int* __restrict__ best,
                                                                          unsigned char* __restrict__ inliers) {
    __shared__ unsigned long long red[kSelectThreads];
    const int tid = threadIdx.x;
    unsigned long long key = 0;                                 // 0: no candidate seen (a real slot's low word is never 0)
    for (long s = tid; s < (long)H * kCands; s += kSelectThreads) {
        const int h = (int)(s / kCands), c = (int)(s % kCands);
        if (c >= nsol[h]) continue;
        const int n = counts[s] > 0 ? counts[s] : 0;
        const unsigned long long k = ((unsigned long long)n << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)s);
        key = k > key ? k : key;
    }
    red[tid] = key;
    __syncthreads();
    for (int w = kSelectThreads / 2; w > 0; w >>= 1) {
        if (tid < w) red[tid] = red[tid + w] > red[tid] ? red[tid + w] : red[tid];
        __syncthreads();
    }
    key = red[0];
    const bool any = key != 0;
    const unsigned slot = 0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull);
    double e[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) e[i] = any ? cand[(size_t)slot * 9 + i] : 0.0;
    if (tid == 0) {
        for (int i = 0; i < 9; ++i) E[i] = e[i];
        best[0] = any ? (int)(key >> 32) : 0;
        best[1] = any ? (int)(slot / kCands) : -1;
        best[2] = any ? (int)(slot % kCands) : -1;
    }
    for (int i = tid; i < N; i += kSelectThreads)
        inliers[i] = any && sampson_inlier(e, x0[2 * (size_t)i], x0[2 * (size_t)i + 1], x1[2 * (size_t)i], x1[2 * (size_t)i + 1], thr2) ? 1 : 0;
}

bool pose_shape_ok(int N, int H) { return N >= 5 && N <= kMaxN && H >= 1 && H <= kMaxH; }

// car_essential_ransac's workspace: cand [H][10][9] doubles | nsol [H] | counts [H][10] | hyp_best [H] ints, each piece of whole 16 bytes
struct PoseWork { double* cand; int *nsol, *counts, *hyp_best; size_t bytes; };
PoseWork pose_work(int H, void* work = nullptr) {
    Carver c(work, 16 / sizeof(int));
    return {c.take<double>((size_t)H * kCands * 9, 16 / sizeof(double)), c.take<int>(H), c.take<int>((size_t)H * kCands), c.take<int>(H), c.bytes()};
}

}  // namespace

extern "C" size_t car_essential_workspace_bytes(int N, int H) {
    if (!pose_shape_ok(N, H)) {
        car_set_error("car_essential_workspace_bytes: N = %d, H = %d; need 5 <= N <= %d matches and 1 <= H <= %d hypotheses", N, H, kMaxN, kMaxH);
        return 0;
    }
    return pose_work(H).bytes;
}

#define POSE_REQUIRE_SHAPE(who)                                                                                              \
    CAR_REQUIRE(N >= 5 && N <= kMaxN, who ": N = %d, the five-point solver needs 5 <= N <= %d matches", N, kMaxN);           \
    CAR_REQUIRE(H >= 1 && H <= kMaxH, who ": H = %d, need 1 <= H <= %d hypotheses", H, kMaxH)

extern "C" int car_essential_solve(const double* x0, const double* x1, int N, const int* samples, int H, double* cand, int* nsol,
                                   void* stream) {
    CAR_REQUIRE(x0 && x1 && samples && cand && nsol, "car_essential_solve: null pointer");
    POSE_REQUIRE_SHAPE("car_essential_solve");
    const size_t lds = (size_t)kSolveLanes * kSolveSlots * sizeof(double);
    CAR_LAUNCH_LDS("car_essential_solve", essential_solve_kernel, dim3(car_div_up(H, kSolveLanes)), dim3(kSolveLanes), lds,
                   (hipStream_t)stream, x0, x1, N, samples, H, cand, nsol);
    return CAR_OK;
}

extern "C" int car_essential_score(const double* x0, const double* x1, int N, const double* cand, const int* nsol, int H, double thresh,
                                   int* counts, int* hyp_best, void* stream) {
    CAR_REQUIRE(x0 && x1 && cand && nsol && counts && hyp_best, "car_essential_score: null pointer");
    POSE_REQUIRE_SHAPE("car_essential_score");
    CAR_REQUIRE(thresh > 0.0 && isfinite(thresh), "car_essential_score: thresh = %g, need a finite value > 0", thresh);
    hipLaunchKernelGGL(essential_score_kernel, dim3(car_div_up(H, kScoreHyp)), dim3(kScoreThreads), 0, (hipStream_t)stream, x0, x1, N, cand,
                       nsol, H, thresh * thresh, counts, hyp_best);
    CAR_CHECK_LAUNCH("car_essential_score");
    return CAR_OK;
}

extern "C" int car_essential_select(const double* x0, const double* x1, int N, const double* cand, const int* nsol, const int* counts,
                                    int H, double thresh, double* E, int* best, unsigned char* inliers, void* stream) {
    CAR_REQUIRE(x0 && x1 && cand && nsol && counts && E && best && inliers, "car_essential_select: null pointer");
    POSE_REQUIRE_SHAPE("car_essential_select");
    CAR_REQUIRE(thresh > 0.0 && isfinite(thresh), "car_essential_select: thresh = %g, need a finite value > 0", thresh);
    hipLaunchKernelGGL(essential_select_kernel, dim3(1), dim3(kSelectThreads), 0, (hipStream_t)stream, x0, x1, N, cand, nsol, counts, H,
                       thresh * thresh, E, best, inliers);
    CAR_CHECK_LAUNCH("car_essential_select");
    return CAR_OK;
}

extern "C" int car_essential_ransac(const double* x0, const double* x1, int N, const int* samples, int H, double thresh, double* E,
                                    int* best, unsigned char* inliers, void* work, size_t work_bytes, void* stream) {
    CAR_REQUIRE(x0 && x1 && samples && E && best && inliers && work, "car_essential_ransac: null pointer");
    POSE_REQUIRE_SHAPE("car_essential_ransac");
    CAR_REQUIRE(thresh > 0.0 && isfinite(thresh), "car_essential_ransac: thresh = %g, need a finite value > 0", thresh);
    const size_t need = car_essential_workspace_bytes(N, H);
    CAR_REQUIRE(work_bytes >= need, "car_essential_ransac: workspace holds %zu bytes, need %zu (car_essential_workspace_bytes)", work_bytes, need);
    CAR_REQUIRE(((size_t)work & 15) == 0, "car_essential_ransac: workspace is not 16-byte aligned");
    const PoseWork w = pose_work(H, work);
    CAR_TRY(car_essential_solve(x0, x1, N, samples, H, w.cand, w.nsol, stream));
    CAR_TRY(car_essential_score(x0, x1, N, w.cand, w.nsol, H, thresh, w.counts, w.hyp_best, stream));
    return car_essential_select(x0, x1, N, w.cand, w.nsol, w.counts, H, thresh, E, best, inliers, stream);
}
