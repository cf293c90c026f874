// Polycrystal moduli of elasticity tensors (include/matten_hip.h, "Polycrystal bounds and the self-consistent estimate"):
// the Hashin-Shtrikman bounds and the self-consistent (Kroener / Hershey / Willis) estimate of the bulk and shear modulus
// of an untextured aggregate of equiaxed grains, from the Kelvin decomposition that matten_elastic_kelvin wrote.
//   polycrystal_kernel     : the four bounds, the self-consistent pair, the comparison media, status and iterations
//   polycrystal_bwd_kernel : the adjoint of the self-consistent pair by the implicit-function theorem
// The reference hands back ElasticTensor(t) (predict.py:217-218) and its users loop over the crystals on the host.  One
// crystal per thread, fp64, everything in registers.
//
// One function carries both: with the isotropic comparison medium (K0, G0), Hill's polarisation tensor P of a sphere in it,
// R = C^ - iso(K0, G0) and A = (1 + P R)^-1,  F_K = c_J(C^ A) / 3 c_J(A),  F_G = c_K(C^ A) / 2 c_K(A).  With
// C* = P^-1 - iso(K0, G0) = a J + b K_d, a = 4 G0, b = G0 (9 K0 + 8 G0) / 3 (K0 + 2 G0), and M = (C^ + C*)^-1:
//   A = M P^-1  and  C^ A = P^-1 - C* M P^-1,  so with m_J = u^T M u, m_K = (tr M - m_J) / 5:
//   F_K = 1 / 3 m_J - a / 3,   F_G = 1 / 2 m_K - b / 2.
// The forward never inverts a matrix: C^ + C* = (C^ + b 1) + (a - b) u u^T is a rank-one update of a matrix whose
// eigen-decomposition is known (moduli l_k, weights w_k = (U_k . u)^2), so with r_k = 1 / (l_k + b), s = sum_k w_k r_k:
//   F_K = (1 / s - b) / 3,   5 m_K = sum_k (1 - w_k) r_k - (a - b) sum_k w_k (r_k - s)^2 / (1 + (a - b) s)
// (Sherman-Morrison; the variance form has no cancellation where the dilatation sits in one mode, as in every cubic
// crystal).  12 doubles of state per crystal; a point of a search is 12 divisions.  The adjoint has no decomposition to
// work from (its signature is that of a backward: the input, the forward's outputs, the upstream gradient), so it inverts
// the symmetric positive definite C^ + C* at the fixed point by Cholesky, every index a compile-time constant.
#include "common.h"

namespace {

constexpr int PC_THREADS = 64;
constexpr double PC_SQRT2 = 1.4142135623730951;       // fp64(sqrt 2)
constexpr double PC_RSQRT3 = 0.57735026918962573;     // fp64(1 / sqrt 3)
// the searches along the frontiers (the same constants in matten_amd/elastic.py)
constexpr double PC_EDGE = 1e-12;
constexpr double PC_GOLDEN = 0.6180339887498949;
constexpr int PC_GOLDEN_STEPS = 60;

__device__ __forceinline__ bool pc_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }   // false for NaN
__device__ __forceinline__ constexpr double pc_mandel(int i, int j) {
    return (i < 3 && j < 3) ? 1.0 : ((i >= 3 && j >= 3) ? 2.0 : PC_SQRT2);
}

// b of C* = 4 G0 J + b K_d
__device__ __forceinline__ double pc_bstar(double K0, double G0) { return G0 * (9.0 * K0 + 8.0 * G0) / (3.0 * (K0 + 2.0 * G0)); }

// F(C^; K0, G0) from the spectrum (header comment)
__device__ __forceinline__ void pc_F(const double (&lam)[6], const double (&w)[6], double K0, double G0, double& FK, double& FG) {
    const double b = pc_bstar(K0, G0), d = 4.0 * G0 - b;
    double r[6], s = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        r[k] = 1.0 / (lam[k] + b);
        s += w[k] * r[k];
    }
    double dev = 0.0, var = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        dev += (1.0 - w[k]) * r[k];
        var += w[k] * ((r[k] - s) * (r[k] - s));
    }
    const double mk5 = dev - d * var / (1.0 + d * s);
    FK = (1.0 / s - b) / 3.0;
    FG = 2.5 / mk5 - 0.5 * b;
}

// the frontier of the feasible comparison media, parametrised by G0: the largest K0 that leaves C^ - iso(K0, G0) positive
// semi-definite (lower frontier, 2 G0 < l_min) or the smallest that leaves iso(K0, G0) - C^ so (upper, 2 G0 > l_max)
template <bool UPPER>
__device__ __forceinline__ double pc_frontier_k0(const double (&lam)[6], const double (&w)[6], double G0) {
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) s += w[k] / (UPPER ? 2.0 * G0 - lam[k] : lam[k] - 2.0 * G0);
    return (UPPER ? 2.0 * G0 - 1.0 / s : 2.0 * G0 + 1.0 / s) / 3.0;
}
// grid point i: lower i = 1..M over (0, edge] (i = 0 is G0 = 0, a bracket end that is never evaluated), upper i = 0..M-1
// over [edge, 4 edge], geometric
template <bool UPPER>
__device__ __forceinline__ double pc_grid(double edge, int i, int M) {
    return UPPER ? edge * exp2(2.0 * (double)i / (double)(M - 1)) : edge * ((double)i / (double)M);
}
template <bool UPPER>
__device__ __forceinline__ bool pc_better(double f, double best) { return UPPER ? f < best : f > best; }   // a NaN never wins

// One bound: the best point visited so far and where.  Every point visited is feasible, so `value` is a bound wherever
// the search ends.
struct pc_best {
    double value, K0, G0;
};
template <bool UPPER>
__device__ __forceinline__ bool pc_keep(pc_best& best, double f, double K0, double G0) {
    const bool take = pc_better<UPPER>(f, best.value);
    best.value = take ? f : best.value;
    best.K0 = take ? K0 : best.K0;
    best.G0 = take ? G0 : best.G0;
    return take;
}

// PC_GOLDEN_STEPS golden-section steps on F_K (Q = 0) or F_G (Q = 1) in [a, b]
template <bool UPPER, int Q>
__device__ __forceinline__ void pc_golden(const double (&lam)[6], const double (&w)[6], double a, double b, pc_best& best) {
    double x1 = b - PC_GOLDEN * (b - a), x2 = a + PC_GOLDEN * (b - a), K0, FK, FG;
    K0 = pc_frontier_k0<UPPER>(lam, w, x1);
    pc_F(lam, w, K0, x1, FK, FG);
    double f1 = Q == 0 ? FK : FG;
    pc_keep<UPPER>(best, f1, K0, x1);
    K0 = pc_frontier_k0<UPPER>(lam, w, x2);
    pc_F(lam, w, K0, x2, FK, FG);
    double f2 = Q == 0 ? FK : FG;
    pc_keep<UPPER>(best, f2, K0, x2);
#pragma unroll 1
    for (int step = 0; step < PC_GOLDEN_STEPS; ++step) {
        const bool left = pc_better<UPPER>(f1, f2);   // the optimum is in [a, x2]
        b = left ? x2 : b;
        a = left ? a : x1;
        const double xn = left ? b - PC_GOLDEN * (b - a) : a + PC_GOLDEN * (b - a);
        K0 = pc_frontier_k0<UPPER>(lam, w, xn);
        pc_F(lam, w, K0, xn, FK, FG);
        const double fn = Q == 0 ? FK : FG;
        pc_keep<UPPER>(best, fn, K0, xn);
        const double o1 = x1, of1 = f1;
        x1 = left ? xn : x2;
        f1 = left ? fn : f2;
        x2 = left ? o1 : xn;
        f2 = left ? of1 : fn;
    }
}

// the two bounds of one frontier: one pass over the grid serves both, then one golden-section search each in the bracket
// of the winner's two neighbours
template <bool UPPER>
__device__ __forceinline__ void pc_bounds(const double (&lam)[6], const double (&w)[6], int M, pc_best& bk, pc_best& bg) {
    const double inf = __longlong_as_double(0x7ff0000000000000LL), nan = __longlong_as_double(0x7ff8000000000000LL);
    const double edge = UPPER ? 0.5 * lam[5] * (1.0 + PC_EDGE) : 0.5 * lam[0] * (1.0 - PC_EDGE);
    const int first = UPPER ? 0 : 1, last = UPPER ? M - 1 : M;
    bk.value = bg.value = UPPER ? inf : -inf;
    bk.K0 = bk.G0 = bg.K0 = bg.G0 = nan;
    int ik = first, ig = first;
#pragma unroll 1
    for (int i = first; i <= last; ++i) {
        const double G0 = pc_grid<UPPER>(edge, i, M), K0 = pc_frontier_k0<UPPER>(lam, w, G0);
        double FK, FG;
        pc_F(lam, w, K0, G0, FK, FG);
        ik = pc_keep<UPPER>(bk, FK, K0, G0) ? i : ik;
        ig = pc_keep<UPPER>(bg, FG, K0, G0) ? i : ig;
    }
    pc_golden<UPPER, 0>(lam, w, pc_grid<UPPER>(edge, max(ik - 1, 0), M), pc_grid<UPPER>(edge, min(ik + 1, last), M), bk);
    pc_golden<UPPER, 1>(lam, w, pc_grid<UPPER>(edge, max(ig - 1, 0), M), pc_grid<UPPER>(edge, min(ig + 1, last), M), bg);
}

// out [n,6] = k_hs_lower, g_hs_lower, k_sc, g_sc, k_hs_upper, g_hs_upper; media [n,8] = (K0, G0) of k_hs_lower, g_hs_lower,
// k_hs_upper, g_hs_upper; status [n,2] = status, iterations of the self-consistent loop.  Flag bit 0 or a decomposition
// that is not finite: NaN, status -1; flag bit 1 or a smallest modulus that is not > 0: NaN, status 2.
__global__ void __launch_bounds__(PC_THREADS) polycrystal_kernel(const int32_t* __restrict__ flags, const double* __restrict__ moduli,
                                                                 const double* __restrict__ vectors, int64_t n, int hs_grid,
                                                                 double sc_tol, int sc_max_iter, double* __restrict__ out,
                                                                 double* __restrict__ media, int32_t* __restrict__ status) {
    const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= n) return;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);

    double lam[6], w[6];
    const int fl = flags[row];
    bool ok = (fl & 1) == 0;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        lam[k] = moduli[row * 6 + k];
        const double tr = (vectors[row * 36 + k] + vectors[row * 36 + 6 + k]) + vectors[row * 36 + 12 + k];   // U_0k + U_1k + U_2k
        w[k] = tr * tr / 3.0;
        ok = ok && pc_finite(lam[k]) && pc_finite(w[k]);
    }
    if (!(ok && (fl & 2) == 0 && lam[0] > 0.0)) {
#pragma unroll
        for (int q = 0; q < 6; ++q) out[row * 6 + q] = nan;
        if (media) {
#pragma unroll
            for (int q = 0; q < 8; ++q) media[row * 8 + q] = nan;
        }
        status[row * 2] = ok ? 2 : -1;
        status[row * 2 + 1] = 0;
        return;
    }

    // ---- the self-consistent pair: (K, G) <- F(C^; K, G) from the Voigt pair
    double wl = 0.0, tr = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        wl += w[k] * lam[k];
        tr += lam[k];
    }
    double K = wl / 3.0, G = (tr - wl) / 10.0;
    int st = 1, it = 0;
#pragma unroll 1
    while (it < sc_max_iter) {
        double Kn, Gn;
        pc_F(lam, w, K, G, Kn, Gn);
        ++it;
        const bool done = fabs(Kn - K) + fabs(Gn - G) <= sc_tol * (Kn + Gn);
        K = Kn, G = Gn;
        if (done) {
            st = 0;
            break;
        }
    }

    // ---- the Hashin-Shtrikman bounds: the best feasible medium along each frontier, for K and for G
    pc_best lo_k, lo_g, up_k, up_g;
    pc_bounds<false>(lam, w, hs_grid, lo_k, lo_g);
    pc_bounds<true>(lam, w, hs_grid, up_k, up_g);

    out[row * 6 + 0] = lo_k.value, out[row * 6 + 1] = lo_g.value;
    out[row * 6 + 2] = K, out[row * 6 + 3] = G;
    out[row * 6 + 4] = up_k.value, out[row * 6 + 5] = up_g.value;
    if (media) {
        media[row * 8 + 0] = lo_k.K0, media[row * 8 + 1] = lo_k.G0, media[row * 8 + 2] = lo_g.K0, media[row * 8 + 3] = lo_g.G0;
        media[row * 8 + 4] = up_k.K0, media[row * 8 + 5] = up_k.G0, media[row * 8 + 6] = up_g.K0, media[row * 8 + 7] = up_g.G0;
    }
    status[row * 2] = st;
    status[row * 2 + 1] = it;
}

// The adjoint of (k_sc, g_sc).  x = (K, G) solves x = F(C^; x), so g_C^ = (dF/dC^)^T l with (1 - dF/dx)^T l = g.  With
// M = (C^ + C*)^-1 at the fixed point, v = M u, m_J = u . v, q = v . v, t2 = tr M^2, m_K = (tr M - m_J) / 5:
//   dF_K/dC^ = v v^T / 3 m_J^2,   dF_G/dC^ = (M^2 - v v^T) / 10 m_K^2              (dM = -M dC^ M)
//   dF_K/da = 0,  dF_K/db = (q - m_J^2) / 3 m_J^2,  dF_G/da = (q - m_J^2) / 10 m_K^2,
//   dF_G/db = (t2 - 2q + m_J^2) / 10 m_K^2 - 1/2                                      (dM = -M (da J + db K_d) M)
//   da/dG = 4,  db/dK = 10 G^2 / 3 (K + 2G)^2,  db/dG = (9 K^2 + 16 K G + 16 G^2) / 3 (K + 2G)^2:  analytic throughout.
// g_voigt = D g_C^ D, symmetric, every element written.  A row whose status is neither 0 nor 1, with flag bit 0, or with a
// value that is not finite gets exact zeros by a select.  A row that stopped at the iteration cap is differentiated as if
// its last iterate were the fixed point.
__global__ void __launch_bounds__(PC_THREADS) polycrystal_bwd_kernel(const double* __restrict__ voigt, const int32_t* __restrict__ flags,
                                                                     const double* __restrict__ out, const int32_t* __restrict__ status,
                                                                     const double* __restrict__ g_sc, int64_t n,
                                                                     double* __restrict__ g_voigt) {
    const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= n) return;
    const double* p = voigt + row * 36;
    const double K = out[row * 6 + 2], G = out[row * 6 + 3];
    const int st = status[row * 2];
    bool ok = (st == 0 || st == 1) && (flags[row] & 1) == 0 && pc_finite(K) && pc_finite(G);
    const double a = 4.0 * G, b = pc_bstar(K, G);

    // B = C^ + a J + b K_d = C^ + b 1 + (a - b) J, lower triangle
    double L[6][6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
#pragma unroll
        for (int j = 0; j <= i; ++j) {
            const double c = pc_mandel(i, j) * (0.5 * (p[i * 6 + j] + p[j * 6 + i]));
            ok = ok && pc_finite(c);
            L[i][j] = c + (i == j ? b : 0.0) + (i < 3 ? (a - b) / 3.0 : 0.0);   // (j <= i < 3: the J block)
        }
    }
    // Cholesky in place: B = L L^T
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double s = L[j][j];
#pragma unroll
        for (int k = 0; k < j; ++k) s -= L[j][k] * L[j][k];
        ok = ok && (s > 0.0);
        L[j][j] = sqrt(s);
        const double inv = 1.0 / L[j][j];
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
            double t = L[i][j];
#pragma unroll
            for (int k = 0; k < j; ++k) t -= L[i][k] * L[j][k];
            L[i][j] = t * inv;
        }
    }
    // X = L^-1 (lower), then M = X^T X (upper triangle mirrored)
    double X[6][6];
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        X[j][j] = 1.0 / L[j][j];
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
            double t = 0.0;
#pragma unroll
            for (int k = j; k < i; ++k) t += L[i][k] * X[k][j];
            X[i][j] = -t / L[i][i];
        }
    }
    double M[6][6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
#pragma unroll
        for (int j = i; j < 6; ++j) {
            double t = 0.0;
#pragma unroll
            for (int k = j; k < 6; ++k) t += X[k][i] * X[k][j];
            M[i][j] = M[j][i] = t;
        }
    }

    double v[6], mj = 0.0, q = 0.0, t2 = 0.0, trm = 0.0;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        v[i] = ((M[i][0] + M[i][1]) + M[i][2]) * PC_RSQRT3;
        q += v[i] * v[i];
        trm += M[i][i];
#pragma unroll
        for (int j = 0; j < 6; ++j) t2 += M[i][j] * M[i][j];
    }
    mj = ((v[0] + v[1]) + v[2]) * PC_RSQRT3;
    const double mk = (trm - mj) / 5.0;
    const double ik = 1.0 / (3.0 * mj * mj), ig = 1.0 / (10.0 * mk * mk);
    const double fk_b = (q - mj * mj) * ik, fg_a = (q - mj * mj) * ig, fg_b = (t2 - 2.0 * q + mj * mj) * ig - 0.5;
    const double den = 3.0 * (K + 2.0 * G) * (K + 2.0 * G);
    const double b_k = 10.0 * G * G / den, b_g = (9.0 * K * K + 16.0 * K * G + 16.0 * G * G) / den;
    const double j11 = fk_b * b_k, j12 = fk_b * b_g, j21 = fg_b * b_k, j22 = 4.0 * fg_a + fg_b * b_g;
    const double det = (1.0 - j11) * (1.0 - j22) - j12 * j21;
    const double gk = g_sc[row * 2], gg = g_sc[row * 2 + 1];
    const double lk = (gk * (1.0 - j22) + j21 * gg) / det * ik, lg = ((1.0 - j11) * gg + j12 * gk) / det * ig;

#pragma unroll
    for (int i = 0; i < 6; ++i) {
#pragma unroll
        for (int j = i; j < 6; ++j) {
            double m2 = 0.0;
#pragma unroll
            for (int k = 0; k < 6; ++k) m2 += M[i][k] * M[k][j];
            const double vv = v[i] * v[j];
            const double g = pc_mandel(i, j) * (lk * vv + lg * (m2 - vv));
            const double o = ok && pc_finite(g) ? g : 0.0;
            g_voigt[row * 36 + i * 6 + j] = o;
            if (j != i) g_voigt[row * 36 + j * 6 + i] = o;
        }
    }
}

}  // namespace

static bool polycrystal_n_ok(int64_t n) { return n >= 0 && n <= (int64_t)0x7fffffff * PC_THREADS; }

extern "C" int matten_elastic_polycrystal(const double* voigt, const int32_t* flags, const double* moduli, const double* vectors,
                                          int64_t n, int hs_grid, double sc_tol, int sc_max_iter, double* out, double* media,
                                          int32_t* status, matten_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!polycrystal_n_ok(n) || hs_grid < 2 || !(sc_tol > 0.0) || !(sc_tol <= 1.7976931348623157e308) || sc_max_iter < 1)
        return MATTEN_EINVAL;
    if (n == 0) return MATTEN_OK;
    if (!voigt || !flags || !moduli || !vectors || !out || !status) return MATTEN_EINVAL;
    // (voigt is part of the entry's contract -- the tensor that moduli and vectors decompose -- but the kernel needs only them)
    polycrystal_kernel<<<(unsigned)matten_cdiv(n, PC_THREADS), PC_THREADS, 0, stream>>>(flags, moduli, vectors, n, hs_grid, sc_tol,
                                                                                       sc_max_iter, out, media, status);
    MATTEN_LAUNCH_CHECK();
    return MATTEN_OK;
}

extern "C" int matten_elastic_polycrystal_bwd(const double* voigt, const int32_t* flags, const double* out, const int32_t* status,
                                              const double* g_sc, int64_t n, double* g_voigt, matten_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!polycrystal_n_ok(n)) return MATTEN_EINVAL;
    if (n == 0) return MATTEN_OK;
    if (!voigt || !flags || !out || !status || !g_sc || !g_voigt) return MATTEN_EINVAL;
    polycrystal_bwd_kernel<<<(unsigned)matten_cdiv(n, PC_THREADS), PC_THREADS, 0, stream>>>(voigt, flags, out, status, g_sc, n, g_voigt);
    MATTEN_LAUNCH_CHECK();
    return MATTEN_OK;
}
