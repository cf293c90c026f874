// Elastic waves per propagation direction beyond the phase velocities (include/matten_hip.h, "Group velocities,
// polarisations and phonon focusing"): the eigenvectors of the Christoffel matrix that elastic_acoustic_kernel discards.
//   elastic_waves_kernel : per direction and branch the polarisation, the group velocity, the power-flow angle, the
//                          longitudinal character and the focusing Jacobian; per crystal the largest power-flow angle and
//                          the smallest |Jacobian| of each branch, the degenerate modes and the unstable directions
// The launch shape, the symmetrised Voigt matrix, the Christoffel matrix, the Jacobi iteration and the stability rule are
// those of elastic_acoustic_kernel (csrc/elastic_dirs.h, csrc/sym3.h): the eigenvalues here are that kernel's.  All
// arithmetic is fp64 in registers with compile-time indices: no scratch memory.  No atomics; every reduction runs in a
// fixed order (lane-strided, xor butterfly in the wave, the four waves in index order): two calls give the same bits.
//
// Every contraction with C_ijkl goes through one 6x6 product.  With the Voigt vector of the symmetrised dyad of a and b,
//   w(a,b) = (a0 b0, a1 b1, a2 b2, a1 b2 + a2 b1, a0 b2 + a2 b0, a0 b1 + a1 b0),   sigma(a,b) = C w(a,b)  (a "stress"),
// sigma(a,b)_ij = sum_kl C_ijkl a_k b_l, and for a unit direction n, a frame vector e and a polarisation u:
//   Gamma u            = sigma(u,n) n
//   P                  = sigma(u,n) u                      (the group velocity is (s / v) P)
//   dGamma u           = sigma(u,n) e + sigma(u,e) n       (dGamma = the derivative of Gamma along e)
//   dP                 = sigma(u,n) du + sigma(du,n) u + sigma(u,e) u
// The second and the third term of dP are different contractions (du sits in another slot of C): they are not one term
// doubled.
#include "common.h"
#include "elastic_dirs.h"
#include "sym3.h"

namespace {

// sigma(a,b) = C w(a,b) as a Voigt 6-vector
__device__ __forceinline__ void dyad_stress(const double (&C)[6][6], V3 a, V3 b, double (&sg)[6]) {
    const double w[6] = {a.x * b.x, a.y * b.y, a.z * b.z, fma(a.y, b.z, a.z * b.y), fma(a.x, b.z, a.z * b.x),
                         fma(a.x, b.y, a.y * b.x)};
    matvec6(C, w, sg);
}
// the symmetric 3x3 matrix held in the Voigt 6-vector sg, applied to x
__device__ __forceinline__ V3 stress_apply(const double (&sg)[6], V3 x) {
    return {sg[0] * x.x + sg[5] * x.y + sg[4] * x.z, sg[5] * x.x + sg[1] * x.y + sg[3] * x.z,
            sg[4] * x.x + sg[3] * x.y + sg[2] * x.z};
}
__device__ __forceinline__ void store3(double* __restrict__ o, V3 a) { o[0] = a.x, o[1] = a.y, o[2] = a.z; }

constexpr double SIGN_EPS = 1e-9;   // below this |u.n| (then |u.e1|) does not decide the sign of a polarisation

// The derivative of the unit group direction g^ of branch K along the frame vector e.  u[m] are the three polarisations,
// lam their eigenvalues, sn = sigma(u_K, n), P = sn u_K, g = (s / v) P, gh = g / |g|.
template <int K>
__device__ __forceinline__ V3 group_dir_derivative(const double (&C)[6][6], V3 n, V3 e, const V3 (&u)[3], const double (&lam)[3],
                                                   const double (&sn)[6], V3 g, V3 gh, double g_abs, double v, double s) {
    constexpr int M1 = (K + 1) % 3, M2 = (K + 2) % 3;
    double se[6];
    dyad_stress(C, u[K], e, se);
    const V3 dGu = add3(stress_apply(sn, e), stress_apply(se, n));   // dGamma u_K
    const double dlam = dot3(u[K], dGu);
    const V3 du = add3(scale3(dot3(u[M1], dGu) / (lam[K] - lam[M1]), u[M1]), scale3(dot3(u[M2], dGu) / (lam[K] - lam[M2]), u[M2]));
    const double dv = s * dlam / (2.0 * v);
    double sd[6];
    dyad_stress(C, du, n, sd);
    const V3 dP = add3(add3(stress_apply(sn, du), stress_apply(sd, u[K])), stress_apply(se, u[K]));
    const V3 dg = add3(scale3(s / v, dP), scale3(-dv / v, g));
    return scale3(1.0 / g_abs, add3(dg, scale3(-dot3(gh, dg), gh)));
}

// Branch K of one direction: writes its rows of pol / group / scal (where asked for) and hands back psi and |J| for the
// extremes (NaN where undefined).  `ok`: the direction is stable.  -> whether the mode is degenerate.
template <int K>
__device__ __forceinline__ bool wave_mode(const double (&C)[6][6], V3 n, V3 e1, V3 e2, const V3 (&u)[3], const double (&lam)[3],
                                          bool ok, double s, double deg_tol, double* __restrict__ pol,
                                          double* __restrict__ group, double* __restrict__ scal, double& psi_out,
                                          double& jabs_out) {
    constexpr int M1 = (K + 1) % 3, M2 = (K + 2) % 3;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    const double gap = fmin(fabs(lam[K] - lam[M1]), fabs(lam[K] - lam[M2])) / lam[2];
    const bool degenerate = ok && gap < deg_tol;
    const bool defined = ok && !degenerate;
    const double v = sqrt(lam[K] * s);

    // the sign of u: u.n >= 0; undecided there, u.e1 >= 0; undecided there too, u.e2 >= 0
    const double un = dot3(u[K], n), u1 = dot3(u[K], e1), u2 = dot3(u[K], e2);
    const double decide = fabs(un) > SIGN_EPS ? un : (fabs(u1) > SIGN_EPS ? u1 : u2);
    const double sign = decide < 0.0 ? -1.0 : 1.0;

    double sn[6];
    dyad_stress(C, u[K], n, sn);
    const V3 P = stress_apply(sn, u[K]);
    const V3 g = scale3(s / v, P);
    const double g_abs = sqrt(dot3(g, g));
    const V3 gh = scale3(1.0 / g_abs, g);
    const double psi = acos(fmin(1.0, v / g_abs));
    const V3 d1 = group_dir_derivative<K>(C, n, e1, u, lam, sn, g, gh, g_abs, v, s);
    const V3 d2 = group_dir_derivative<K>(C, n, e2, u, lam, sn, g, gh, g_abs, v, s);
    const double J = dot3(gh, cross3(d1, d2));

    if (pol) store3(pol + K * 3, defined ? scale3(sign, u[K]) : V3{nan, nan, nan});
    if (group) store3(group + K * 3, defined ? g : V3{nan, nan, nan});
    if (scal) {
        double* o = scal + K * 5;
        o[0] = ok ? v : nan;
        o[1] = defined ? g_abs : nan;
        o[2] = defined ? psi : nan;
        o[3] = defined ? un * un : nan;
        o[4] = defined ? J : nan;
    }
    psi_out = defined ? psi : nan;
    jabs_out = defined ? fabs(J) : nan;
    return degenerate;
}

// One workgroup per crystal, a lane per direction in strides of DIR_THREADS.
__global__ void __launch_bounds__(DIR_THREADS) elastic_waves_kernel(
    const double* __restrict__ voigt, const int32_t* __restrict__ flags, const double* __restrict__ density,
    const double* __restrict__ dirs, int n_dirs, double modulus_unit, double deg_tol, double* __restrict__ pol,
    double* __restrict__ group, double* __restrict__ scal, double* __restrict__ ext, int32_t* __restrict__ arg,
    int32_t* __restrict__ n_degenerate, int32_t* __restrict__ n_unstable) {
    const int64_t b = blockIdx.x;
    const int t = threadIdx.x;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    const double rho = density[b];
    if ((flags[b] & 1) || !(rho > 0.0) || !finite64(rho)) {   // (uniform over the workgroup)
        for (int64_t i = t; i < (int64_t)n_dirs * 9; i += DIR_THREADS) {
            if (pol) pol[b * n_dirs * 9 + i] = nan;
            if (group) group[b * n_dirs * 9 + i] = nan;
        }
        if (scal) {
            for (int64_t i = t; i < (int64_t)n_dirs * 15; i += DIR_THREADS) scal[b * n_dirs * 15 + i] = nan;
        }
        if (t < 6) ext[b * 6 + t] = nan, arg[b * 6 + t] = -1;
        if (t < 3) n_degenerate[b * 3 + t] = -1;
        if (t == 0) n_unstable[b] = -1;
        return;
    }
    double C[6][6];
    load_sym6(voigt + b * 36, C);
    const double s = modulus_unit / rho;

    const double inf = __longlong_as_double(0x7ff0000000000000LL);
    // block_best's layout, minima at even and maxima at odd positions: the smallest |J| of branch k at 2 k, its psi_max at 2 k + 1
    Ext best[6] = {{inf, EXT_NONE}, {-inf, EXT_NONE}, {inf, EXT_NONE}, {-inf, EXT_NONE}, {inf, EXT_NONE}, {-inf, EXT_NONE}};
    int count[4] = {0, 0, 0, 0};   // degenerate modes per branch, unstable directions
    for (int d = t; d < n_dirs; d += DIR_THREADS) {
        const V3 n = load_dir(dirs, d);
        const double nv[3] = {n.x, n.y, n.z};
        double G[3][3], lam[3], U[3][3];   // column k of U = u_k
        christoffel(C, nv, G);
        sym3_eig<true>(G, lam, U);
        const bool ok = stable3(lam);
        sort3(lam, U);
        const V3 u[3] = {{U[0][0], U[1][0], U[2][0]}, {U[0][1], U[1][1], U[2][1]}, {U[0][2], U[1][2], U[2][2]}};
        V3 e1, e2;
        pair_frame(n, e1, e2);
        const int64_t at = b * n_dirs + d;
        double* p = pol ? pol + at * 9 : nullptr;
        double* g = group ? group + at * 9 : nullptr;
        double* q = scal ? scal + at * 15 : nullptr;
        double psi[3], jabs[3];
        count[0] += wave_mode<0>(C, n, e1, e2, u, lam, ok, s, deg_tol, p, g, q, psi[0], jabs[0]) ? 1 : 0;
        count[1] += wave_mode<1>(C, n, e1, e2, u, lam, ok, s, deg_tol, p, g, q, psi[1], jabs[1]) ? 1 : 0;
        count[2] += wave_mode<2>(C, n, e1, e2, u, lam, ok, s, deg_tol, p, g, q, psi[2], jabs[2]) ? 1 : 0;
        count[3] += ok ? 0 : 1;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            best[2 * k] = better<false>(best[2 * k], Ext{jabs[k], d});   // (a NaN compares false: never taken)
            best[2 * k + 1] = better<true>(best[2 * k + 1], Ext{psi[k], d});
        }
    }
    // the counts: integer sums by the xor butterfly in the wave, then the four waves in index order through LDS
#pragma unroll
    for (int k = 0; k < 4; ++k) {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) count[k] += __shfl_xor(count[k], off, 64);
    }
    __shared__ int sh_count[DIR_THREADS / 64][4];
    if ((t & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) sh_count[t >> 6][k] = count[k];
    }
    // the extremes: block_best (its barrier covers sh_count as well) leaves them interleaved in LDS; the lane that wrote
    // position q moves it to its place in ext / arg [psi_max x 3, min |J| x 3]
    __shared__ double sh_ext[6];
    __shared__ int32_t sh_arg[6];
    block_best<6, true>(best, sh_ext, sh_arg, t);
    if (t < 6) {
        const int to = (t & 1) ? (t >> 1) : 3 + (t >> 1);
        ext[b * 6 + to] = sh_ext[t];
        arg[b * 6 + to] = sh_arg[t];
    }
    if (t < 4) {
        int total = sh_count[0][t];
#pragma unroll
        for (int w = 1; w < DIR_THREADS / 64; ++w) total += sh_count[w][t];
        if (t < 3) n_degenerate[b * 3 + t] = total;
        else n_unstable[b] = total;
    }
}

}  // namespace

extern "C" int matten_elastic_waves(const double* voigt, const int32_t* flags, const double* density, const double* dirs,
                                    int64_t n, int64_t n_dirs, double modulus_unit, double deg_tol, double* pol, double* group,
                                    double* scal, double* ext, int32_t* arg, int32_t* n_degenerate, int32_t* n_unstable,
                                    matten_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    // (the direction index and d * 3 are 32-bit in the kernel; the output offsets are 64-bit)
    if (n < 0 || n > 0x7fffffff || n_dirs < 1 || n_dirs > 0x7fffffff / 3) return MATTEN_EINVAL;
    if (!(deg_tol >= 0.0) || !(deg_tol <= 1.7976931348623157e308)) return MATTEN_EINVAL;
    if (n == 0) return MATTEN_OK;
    if (!voigt || !flags || !density || !dirs || !ext || !arg || !n_degenerate || !n_unstable) return MATTEN_EINVAL;
    elastic_waves_kernel<<<(unsigned)n, DIR_THREADS, 0, stream>>>(voigt, flags, density, dirs, (int)n_dirs, modulus_unit, deg_tol,
                                                                  pol, group, scal, ext, arg, n_degenerate, n_unstable);
    MATTEN_LAUNCH_CHECK();
    return MATTEN_OK;
}
