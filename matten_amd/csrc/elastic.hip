// Derived elastic properties of predicted elasticity tensors (include/matten_hip.h, "Derived elastic properties").
//   elastic_props_kernel       : Voigt matrix, compliance, the ten scalar moduli and the flags   reference predict.py:217-218
//   elastic_props_bwd_kernel   : its adjoint (gradients of the scalars, the Voigt matrix and the compliance -> the input)
//   elastic_directional_kernel : Young's modulus and linear compressibility over a direction set, with their extremes
//   elastic_pair_kernel        : shear modulus and Poisson's ratio over pairs of perpendicular directions, with their extremes
//   elastic_acoustic_kernel    : the three acoustic phase velocities per direction (Christoffel equation), their extremes
//                                and the sum of v^-3 of the Debye average
//   elastic_directional_bwd_kernel, elastic_acoustic_bwd_kernel : the adjoints of those two (gradients of the maps, the
//                                extremes and the sum of v^-3 -> the compliance / the Voigt matrix)
//   elastic_refine_kernel      : the extremes of the directional and the pair kernel polished off the grid
// The reference wraps every predicted tensor in pymatgen's ElasticTensor (one Python object per crystal); these kernels
// compute what its users read off that object.  All arithmetic is fp64; everything is held in registers with compile-time
// indices, so no kernel here uses scratch memory (hipcc -Rpass-analysis=kernel-resource-usage: DESIGN.md).  Every formula
// that a forward, its adjoint and the refinement share is one helper here: "the same bits" between them is one piece of
// code, not two kept in step.
#include "common.h"
#include "elastic_dirs.h"
#include "sym3.h"

namespace {

// pymatgen's Voigt order xx, yy, zz, yz, xz, xy
__device__ constexpr int VI[6] = {0, 1, 2, 1, 0, 0};
__device__ constexpr int VJ[6] = {0, 1, 2, 2, 2, 1};

__device__ __forceinline__ constexpr int cart(int i, int j, int k, int l) { return ((i * 3 + j) * 3 + k) * 3 + l; }

// (finite64, V3, load_dir, load_sym6, matvec6, pair_frame, the extremes of a workgroup, the Christoffel matrix: csrc/elastic_dirs.h,
// shared with csrc/waves.hip)
__device__ __forceinline__ double dot6(const double (&a)[6], const double (&b)[6]) {
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < 6; ++i) s += a[i] * b[i];
    return s;
}
// v(n): 1 / E(n) = v^T S v, beta(n) = r . v with the compressibility's row sums r
__device__ __forceinline__ void voigt_dyad(V3 n, double (&v)[6]) {
    v[0] = n.x * n.x, v[1] = n.y * n.y, v[2] = n.z * n.z, v[3] = n.y * n.z, v[4] = n.x * n.z, v[5] = n.x * n.y;
}
// w(n,m): 1 / G(n,m) = w^T S w.  The fma of a b + c d is spelled out, here and in frame_dir: left to the compiler, which of
// the two products is rounded before the sum depends on where the expression is inlined, and the pair kernel and the
// refinement, which starts from the pair kernel's winner, must form the same m and the same w.
__device__ __forceinline__ void voigt_pair(V3 n, V3 m, double (&w)[6]) {
    w[0] = 2.0 * n.x * m.x, w[1] = 2.0 * n.y * m.y, w[2] = 2.0 * n.z * m.z;
    w[3] = fma(n.y, m.z, n.z * m.y), w[4] = fma(n.x, m.z, n.z * m.x), w[5] = fma(n.x, m.y, n.y * m.x);
}
__device__ __forceinline__ void compress_rows(const double (&S)[6][6], double (&r)[6]) {
#pragma unroll
    for (int i = 0; i < 6; ++i) r[i] = S[i][0] + S[i][1] + S[i][2];
}
// the direction at the angle (c, s) = (cos, sin) in the frame (e1, e2) of a unit vector (pair_frame, csrc/elastic_dirs.h)
__device__ __forceinline__ V3 frame_dir(double c, double s, V3 e1, V3 e2) {
    return {fma(c, e1.x, s * e2.x), fma(c, e1.y, s * e2.y), fma(c, e1.z, s * e2.z)};
}

// One crystal per thread.  LAYOUT 0: c [n, 81] Cartesian, 1: c [n, 36] Voigt.
template <typename T, int LAYOUT>
__global__ void __launch_bounds__(64) elastic_props_kernel(const T* __restrict__ c, int64_t n, double* __restrict__ voigt,
                                                           double* __restrict__ compliance, double* __restrict__ props,
                                                           int32_t* __restrict__ flags) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n) return;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);

    // ---- the symmetrised 6x6 matrix: the input is never trusted to be symmetric
    double C[6][6];
    if (LAYOUT == 0) {
        const T* p = c + b * 81;
#pragma unroll
        for (int I = 0; I < 6; ++I) {
#pragma unroll
            for (int J = I; J < 6; ++J) {
                const int i = VI[I], j = VJ[I], k = VI[J], l = VJ[J];
                // the 8 entries equivalent under ij<->ji, kl<->lk, (ij)<->(kl) (entries that coincide are counted twice)
                const double s = (((double)p[cart(i, j, k, l)] + (double)p[cart(j, i, k, l)]) +
                                  ((double)p[cart(i, j, l, k)] + (double)p[cart(j, i, l, k)])) +
                                 (((double)p[cart(k, l, i, j)] + (double)p[cart(k, l, j, i)]) +
                                  ((double)p[cart(l, k, i, j)] + (double)p[cart(l, k, j, i)]));
                C[I][J] = C[J][I] = 0.125 * s;
            }
        }
    } else {
        load_sym6(c + b * 36, C);
    }
    bool ok = true;
#pragma unroll
    for (int I = 0; I < 6; ++I) {
#pragma unroll
        for (int J = I; J < 6; ++J) ok = ok && finite64(C[I][J]);
    }

    // ---- Born stability: un-pivoted LDL^T, positive definite iff every d > 0 (a zero or NaN d fails the comparison, and
    // every later one with it)
    bool pd = true;
    {
        double L[6][6], d[6];
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            double dj = C[j][j];
#pragma unroll
            for (int k = 0; k < j; ++k) dj -= L[j][k] * L[j][k] * d[k];
            d[j] = dj;
            pd = pd && (dj > 0.0);
            const double inv = 1.0 / dj;
#pragma unroll
            for (int i = j + 1; i < 6; ++i) {
                double v = C[i][j];
#pragma unroll
                for (int k = 0; k < j; ++k) v -= L[i][k] * L[j][k] * d[k];
                L[i][j] = v * inv;
            }
        }
    }

    // ---- compliance: Gauss-Jordan on [C | 1] with partial pivoting, rows exchanged by selects (every index is a
    // compile-time constant).  Indefinite matrices (a random-init model) are inverted like any other.
    double A[6][12];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            A[i][j] = C[i][j];
            A[i][6 + j] = i == j ? 1.0 : 0.0;
        }
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        int piv = k;
        double best = fabs(A[k][k]);
#pragma unroll
        for (int i = k + 1; i < 6; ++i) {
            const double v = fabs(A[i][k]);
            const bool take = v > best;      // ties keep the upper row
            best = take ? v : best;
            piv = take ? i : piv;
        }
#pragma unroll
        for (int i = k + 1; i < 6; ++i) {
            const bool sw = piv == i;
#pragma unroll
            for (int j = k; j < 12; ++j) {   // the columns left of k are already 0 in both rows
                const double u = A[k][j], v = A[i][j];
                A[k][j] = sw ? v : u;
                A[i][j] = sw ? u : v;
            }
        }
        ok = ok && (best > 0.0) && finite64(best);
        const double inv = 1.0 / A[k][k];
#pragma unroll
        for (int j = k; j < 12; ++j) A[k][j] *= inv;
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            if (i == k) continue;
            const double f = A[i][k];
#pragma unroll
            for (int j = k; j < 12; ++j) A[i][j] -= f * A[k][j];
        }
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) {
#pragma unroll
        for (int j = 0; j < 6; ++j) ok = ok && finite64(A[i][6 + j]);
    }
#define S_(i, j) A[i][6 + (j)]

    // ---- the ten scalars (units of the input tensor)
    const double c_diag = C[0][0] + C[1][1] + C[2][2], c_off = C[0][1] + C[0][2] + C[1][2], c_sh = C[3][3] + C[4][4] + C[5][5];
    const double s_diag = S_(0, 0) + S_(1, 1) + S_(2, 2), s_off = S_(0, 1) + S_(0, 2) + S_(1, 2),
                 s_sh = S_(3, 3) + S_(4, 4) + S_(5, 5);
    double P[10];
    P[0] = (c_diag + 2.0 * c_off) / 9.0;                              // k_voigt
    P[1] = (c_diag - c_off + 3.0 * c_sh) / 15.0;                      // g_voigt
    P[2] = 1.0 / (s_diag + 2.0 * s_off);                              // k_reuss
    P[3] = 15.0 / (4.0 * s_diag - 4.0 * s_off + 3.0 * s_sh);          // g_reuss
    P[4] = 0.5 * (P[0] + P[2]);                                       // k_vrh
    P[5] = 0.5 * (P[1] + P[3]);                                       // g_vrh
    P[6] = 9.0 * P[4] * P[5] / (3.0 * P[4] + P[5]);                   // y_mod
    P[7] = (3.0 * P[4] - 2.0 * P[5]) / (2.0 * (3.0 * P[4] + P[5]));   // homogeneous_poisson
    P[8] = 5.0 * P[1] / P[3] + P[0] / P[2] - 6.0;                     // universal_anisotropy
    P[9] = P[4] / P[5];                                               // pugh_ratio

    double* vo = voigt + b * 36;
    double* so = compliance + b * 36;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            vo[i * 6 + j] = ok ? C[i][j] : nan;
            so[i * 6 + j] = ok ? S_(i, j) : nan;
        }
    }
#undef S_
#pragma unroll
    for (int q = 0; q < 10; ++q) props[b * 10 + q] = ok ? P[q] : nan;
    flags[b] = (ok ? 0 : 1) | (pd ? 0 : 2);
}

// The adjoint of elastic_props_kernel, one crystal per thread, from what the forward wrote (voigt = the symmetrised C,
// compliance = S, props, flags): upstream gradients of the ten scalars and, optionally, of voigt and compliance -> the
// gradient of the input tensor.  The chain: scalars -> (K, G of the VRH means) -> the four Voigt / Reuss bounds -> the
// entries of C and S the forward summed; S = C^-1 as a general 6x6 gives Cbar -= S^T Sbar S^T; the symmetrisation is
// linear, its transpose spreads H = (Cbar + Cbar^T) / 2 over the positions it averaged.  Only S and one temporary
// T = Sbar S^T stay live (Sbar is made a row at a time, Cbar an entry at a time).  The stored voigt enters no derivative
// (every scalar is linear in C or a function of S and the stored scalars), so the entry checks it and the kernel does not
// take it.  A row with flag bit 0 gets zeros by selects: its NaN never reaches the output.
template <typename T, int LAYOUT>
__global__ void __launch_bounds__(64) elastic_props_bwd_kernel(const double* __restrict__ compliance,
                                                               const double* __restrict__ props,
                                                               const int32_t* __restrict__ flags,
                                                               const double* __restrict__ g_props,
                                                               const double* __restrict__ g_voigt,
                                                               const double* __restrict__ g_compliance, int64_t n,
                                                               T* __restrict__ g_c) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n) return;
    const bool bad = (flags[b] & 1) != 0;

    // ---- the ten scalars' gradients folded into the four bounds, then into the sums the forward took of C and S
    double P[10], gP[10];
#pragma unroll
    for (int q = 0; q < 10; ++q) {
        P[q] = props[b * 10 + q];
        gP[q] = g_props[b * 10 + q];
    }
    const double K = P[4], G = P[5], D = 3.0 * K + G, inv_d2 = 1.0 / (D * D);
    const double k_bar = gP[4] + gP[6] * (9.0 * G * G * inv_d2) + gP[7] * (4.5 * G * inv_d2) + gP[9] / G;
    const double g_bar = gP[5] + gP[6] * (27.0 * K * K * inv_d2) - gP[7] * (4.5 * K * inv_d2) - gP[9] * (K / (G * G));
    const double kv_bar = gP[0] + 0.5 * k_bar + gP[8] / P[2];
    const double gv_bar = gP[1] + 0.5 * g_bar + gP[8] * (5.0 / P[3]);
    const double kr_bar = gP[2] + 0.5 * k_bar - gP[8] * (P[0] / (P[2] * P[2]));
    const double gr_bar = gP[3] + 0.5 * g_bar - gP[8] * (5.0 * P[1] / (P[3] * P[3]));
    const double kr2 = kr_bar * (P[2] * P[2]), gr2 = gr_bar * (P[3] * P[3]) / 15.0;
    const double s_diag_bar = -kr2 - 4.0 * gr2, s_off_bar = -2.0 * kr2 + 4.0 * gr2, s_sh_bar = -3.0 * gr2;
    const double c_diag_bar = kv_bar / 9.0 + gv_bar / 15.0, c_off_bar = 2.0 * kv_bar / 9.0 - gv_bar / 15.0,
                 c_sh_bar = 3.0 * gv_bar / 15.0;

    double S[6][6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
#pragma unroll
        for (int j = 0; j < 6; ++j) S[i][j] = compliance[b * 36 + i * 6 + j];
    }
    // an absent upstream gradient is read from a valid row and replaced by zero with a select: no branch around the loads
    const bool has_gs = g_compliance != nullptr, has_gv = g_voigt != nullptr;
    const double* gs = (has_gs ? g_compliance : compliance) + b * 36;
    const double* gv = (has_gv ? g_voigt : compliance) + b * 36;
    // ---- pass 1: T = Sbar S^T, a row of Sbar at a time (the entries the forward read: diagonal 0..2, the three upper
    // off-diagonals, diagonal 3..5)
    double Tm[6][6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        double row[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            double v = has_gs ? gs[i * 6 + k] : 0.0;
            if (i == k) v += i < 3 ? s_diag_bar : s_sh_bar;
            if (i < k && k < 3) v += s_off_bar;
            row[k] = v;
        }
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            double acc = 0.0;
#pragma unroll
            for (int k = 0; k < 6; ++k) acc += row[k] * S[j][k];
            Tm[i][j] = acc;
        }
    }
    // ---- pass 2: Cbar = g_voigt + (the Voigt bounds' weights) - S^T T and H = (Cbar + Cbar^T) / 2, an entry at a time,
    // each sent straight through the transpose of the symmetrisation.  Layout 0: the mean over the 8 equivalent
    // positions, coinciding ones counted twice, gives a position (i,j,k,l) of the pair (I, J) the weight 1 / (n_I n_J)
    // of H_IJ, n = 1 for a diagonal Cartesian pair (i == j) and 2 otherwise (positions that coincide are written twice
    // with the same value).  Layout 1: H itself.
    T* o = g_c + b * (LAYOUT == 0 ? 81 : 36);
#pragma unroll
    for (int I = 0; I < 6; ++I) {
#pragma unroll
        for (int J = I; J < 6; ++J) {
            double m_ij = 0.0, m_ji = 0.0;
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                m_ij += S[k][I] * Tm[k][J];
                m_ji += S[k][J] * Tm[k][I];
            }
            double c_ij = has_gv ? gv[I * 6 + J] : 0.0;
            double c_ji = has_gv ? gv[J * 6 + I] : 0.0;
            if (I == J) {
                const double w = I < 3 ? c_diag_bar : c_sh_bar;
                c_ij += w;
                c_ji += w;
            }
            if (I < J && J < 3) c_ij += c_off_bar;
            const double h0 = 0.5 * ((c_ij - m_ij) + (c_ji - m_ji));
            const double h = bad ? 0.0 : h0;
            if (LAYOUT == 0) {
                const int i = VI[I], j = VJ[I], k = VI[J], l = VJ[J];
                const T v = (T)((i == j ? 1.0 : 0.5) * (k == l ? 1.0 : 0.5) * h);
                o[cart(i, j, k, l)] = v, o[cart(j, i, k, l)] = v, o[cart(i, j, l, k)] = v, o[cart(j, i, l, k)] = v;
                o[cart(k, l, i, j)] = v, o[cart(k, l, j, i)] = v, o[cart(l, k, i, j)] = v, o[cart(l, k, j, i)] = v;
            } else {
                o[I * 6 + J] = o[J * 6 + I] = (T)h;
            }
        }
    }
}

// ((value, direction index) pairs and the workgroup's winners -- Ext, better, wave_best, block_best, DIR_THREADS, EXT_NONE --
// are csrc/elastic_dirs.h)

// One workgroup per crystal, a lane per direction in strides of DIR_THREADS.
__global__ void __launch_bounds__(DIR_THREADS) elastic_directional_kernel(const double* __restrict__ compliance,
                                                                          const int32_t* __restrict__ flags,
                                                                          const double* __restrict__ dirs, int n_dirs,
                                                                          double* __restrict__ young, double* __restrict__ beta,
                                                                          double* __restrict__ ext, int32_t* __restrict__ arg) {
    const int64_t b = blockIdx.x;
    const int t = threadIdx.x;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    if (flags[b] & 1) {   // (uniform over the workgroup)
        for (int d = t; d < n_dirs; d += DIR_THREADS) {
            if (young) young[b * n_dirs + d] = nan;
            if (beta) beta[b * n_dirs + d] = nan;
        }
        if (t < 4) {
            ext[b * 4 + t] = nan;
            arg[b * 4 + t] = -1;
        }
        return;
    }
    double S[6][6], r[6];
    load_sym6(compliance + b * 36, S);
    compress_rows(S, r);

    const double inf = __longlong_as_double(0x7ff0000000000000LL);
    Ext best[4] = {{inf, EXT_NONE}, {-inf, EXT_NONE}, {inf, EXT_NONE}, {-inf, EXT_NONE}};   // E_min, E_max, beta_min, beta_max
    for (int d = t; d < n_dirs; d += DIR_THREADS) {
        double v[6], Sv[6];
        voigt_dyad(load_dir(dirs, d), v);
        matvec6(S, v, Sv);
        const double E = 1.0 / dot6(v, Sv), bt = dot6(r, v);
        if (young) young[b * n_dirs + d] = E;
        if (beta) beta[b * n_dirs + d] = bt;
        const Ext ce = {E, d}, cb = {bt, d};
        best[0] = better<false>(best[0], ce);
        best[1] = better<true>(best[1], ce);
        best[2] = better<false>(best[2], cb);
        best[3] = better<true>(best[3], cb);
    }
    block_best<4, false>(best, ext + b * 4, arg + b * 4, t);
}

// One workgroup per crystal, a lane per direction n in strides of DIR_THREADS; the lane walks the n_ang directions
// m_k = cos(chi_k) e1 + sin(chi_k) e2 perpendicular to n itself, so the extremes over chi are lane-local.
//   1/G(n,m) = w^T S w,  w = (2 n1 m1, 2 n2 m2, 2 n3 m3, n2 m3 + n3 m2, n1 m3 + n3 m1, n1 m2 + n2 m1)
//   nu(n,m)  = -(v(n)^T S v(m)) / (v(n)^T S v(n))
__global__ void __launch_bounds__(DIR_THREADS) elastic_pair_kernel(const double* __restrict__ compliance,
                                                                   const int32_t* __restrict__ flags,
                                                                   const double* __restrict__ dirs, int n_dirs,
                                                                   const double* __restrict__ cos_sin, int n_ang,
                                                                   double* __restrict__ maps, double* __restrict__ ext,
                                                                   int32_t* __restrict__ arg) {
    const int64_t b = blockIdx.x;
    const int t = threadIdx.x;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    if (flags[b] & 1) {   // (uniform over the workgroup)
        if (maps) {
            for (int64_t i = t; i < (int64_t)n_dirs * 4; i += DIR_THREADS) maps[b * n_dirs * 4 + i] = nan;
        }
        if (t < 4) {
            ext[b * 4 + t] = nan;
            arg[b * 4 + t] = -1;
        }
        return;
    }
    double S[6][6];
    load_sym6(compliance + b * 36, S);

    const double inf = __longlong_as_double(0x7ff0000000000000LL);
    Ext best[4] = {{inf, EXT_NONE}, {-inf, EXT_NONE}, {inf, EXT_NONE}, {-inf, EXT_NONE}};   // G_min, G_max, nu_min, nu_max
    for (int d = t; d < n_dirs; d += DIR_THREADS) {
        const V3 n = load_dir(dirs, d);
        double v[6], Sv[6];
        voigt_dyad(n, v);
        matvec6(S, v, Sv);
        const double q = dot6(v, Sv);
        V3 e1, e2;
        pair_frame(n, e1, e2);

        Ext here[4] = {{inf, EXT_NONE}, {-inf, EXT_NONE}, {inf, EXT_NONE}, {-inf, EXT_NONE}};
        const int base = d * n_ang;
        for (int k = 0; k < n_ang; ++k) {
            const V3 m = frame_dir(cos_sin[2 * (int64_t)k], cos_sin[2 * (int64_t)k + 1], e1, e2);
            double vm[6], w[6], Sw[6];
            voigt_dyad(m, vm);
            voigt_pair(n, m, w);
            matvec6(S, w, Sw);
            const double h = dot6(w, Sw), num = dot6(Sv, vm);
            const Ext cg = {1.0 / h, base + k}, cn = {-num / q, base + k};
            here[0] = better<false>(here[0], cg);
            here[1] = better<true>(here[1], cg);
            here[2] = better<false>(here[2], cn);
            here[3] = better<true>(here[3], cn);
        }
#pragma unroll
        for (int x = 0; x < 4; ++x) {
            if (maps) maps[(b * n_dirs + d) * 4 + x] = here[x].i == EXT_NONE ? nan : here[x].v;
            best[x] = (x & 1) ? better<true>(best[x], here[x]) : better<false>(best[x], here[x]);
        }
    }
    block_best<4, true>(best, ext + b * 4, arg + b * 4, t);
}

// (Gamma_ik = C_ijkl n_j n_l -- christoffel, VOIGT_OF -- and the stability rule stable3 are csrc/elastic_dirs.h; the cyclic
// Jacobi of a symmetric 3x3 matrix -- sym3_eig, sort3 -- is csrc/sym3.h)

// One workgroup per crystal, a lane per direction in strides of DIR_THREADS: Gamma_ik = C_ijkl n_j n_l, its eigenvalues
// by cyclic Jacobi in registers, v_i = sqrt(lambda_i unit / rho) ascending.
__global__ void __launch_bounds__(DIR_THREADS) elastic_acoustic_kernel(const double* __restrict__ voigt,
                                                                       const int32_t* __restrict__ flags,
                                                                       const double* __restrict__ density,
                                                                       const double* __restrict__ dirs, int n_dirs,
                                                                       double modulus_unit, double* __restrict__ vel,
                                                                       double* __restrict__ ext, int32_t* __restrict__ arg,
                                                                       int32_t* __restrict__ n_unstable) {
    const int64_t b = blockIdx.x;
    const int t = threadIdx.x;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    const double rho = density[b];
    if ((flags[b] & 1) || !(rho > 0.0) || !finite64(rho)) {   // (uniform over the workgroup)
        if (vel) {
            for (int64_t i = t; i < (int64_t)n_dirs * 3; i += DIR_THREADS) vel[b * n_dirs * 3 + i] = nan;
        }
        if (t < 3) ext[b * 3 + t] = nan;
        if (t < 2) arg[b * 2 + t] = -1;
        if (t == 0) n_unstable[b] = -1;
        return;
    }
    double C[6][6];
    load_sym6(voigt + b * 36, C);
    const double scale = modulus_unit / rho;

    const double inf = __longlong_as_double(0x7ff0000000000000LL);
    Ext best[2] = {{inf, EXT_NONE}, {-inf, EXT_NONE}};   // v_slow_min, v_fast_max
    double sum = 0.0;
    int bad = 0;
    for (int d = t; d < n_dirs; d += DIR_THREADS) {
        const double n[3] = {dirs[d * 3 + 0], dirs[d * 3 + 1], dirs[d * 3 + 2]};
        double G[3][3], lam[3], U[3][3];
        christoffel(C, n, G);
        sym3_eig<false>(G, lam, U);
        const bool ok = stable3(lam);
        const double lo01 = fmin(lam[0], lam[1]), hi01 = fmax(lam[0], lam[1]);
        const double l0 = fmin(lo01, lam[2]), top = fmax(lo01, lam[2]);
        const double l1 = fmin(hi01, top), l2 = fmax(hi01, top);
        const double v0 = ok ? sqrt(l0 * scale) : nan, v1 = ok ? sqrt(l1 * scale) : nan, v2 = ok ? sqrt(l2 * scale) : nan;
        if (vel) {
            double* o = vel + (b * n_dirs + d) * 3;
            o[0] = v0, o[1] = v1, o[2] = v2;
        }
        bad += ok ? 0 : 1;
        sum += (1.0 / (v0 * v0 * v0) + 1.0 / (v1 * v1 * v1)) + 1.0 / (v2 * v2 * v2);
        const Ext c0 = {v0, d}, c2 = {v2, d};
        best[0] = better<false>(best[0], c0);   // (a NaN compares false: never taken)
        best[1] = better<true>(best[1], c2);
    }
    // the sum in a fixed order: the lane's strided partial sum, an xor butterfly in the wave (a + b = b + a: every lane
    // holds the same bits), the four waves in index order
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        sum += __shfl_xor(sum, off, 64);
        bad += __shfl_xor(bad, off, 64);
    }
    __shared__ double sh_sum[DIR_THREADS / 64];
    __shared__ int sh_bad[DIR_THREADS / 64];
    if ((t & 63) == 0) sh_sum[t >> 6] = sum, sh_bad[t >> 6] = bad;
    block_best<2, true>(best, ext + b * 3, arg + b * 2, t);   // (its barrier covers sh_sum / sh_bad as well)
    if (t == 0) {
        double total = sh_sum[0];
        int n_bad = sh_bad[0];
#pragma unroll
        for (int w = 1; w < DIR_THREADS / 64; ++w) total += sh_sum[w], n_bad += sh_bad[w];
        ext[b * 3 + 2] = total;
        n_unstable[b] = n_bad;
    }
}

// ---------------------------------------------------------------------------------------------------
// the adjoints of the directional and the acoustic kernel (training on directional moduli, sound velocities and the
// Debye temperature): the same launch shape as their forwards, lane-strided partial sums of the gradient's distinct
// entries, combined in a fixed order
// ---------------------------------------------------------------------------------------------------

// position of (i, j), i <= j, in the row-major upper triangle of a symmetric 6x6 matrix (21 entries)
__device__ __forceinline__ constexpr int tri6(int i, int j) { return i * 6 - (i * (i - 1)) / 2 + (j - i); }

// The workgroup's sum of NV lane-partial values in a fixed order: an xor butterfly in the wave (a + b = b + a: every
// lane holds the same bits), then the four waves in index order through LDS.  total[NV] lives in LDS and is complete
// for every thread on return.  No atomics: bitwise reproducible.
template <int NV>
__device__ __forceinline__ void block_sum(double (&a)[NV], double* __restrict__ total, int t) {
    __shared__ double sh[DIR_THREADS / 64][NV];
#pragma unroll
    for (int q = 0; q < NV; ++q) {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) a[q] += __shfl_xor(a[q], off, 64);
    }
    const int wave = t >> 6;
    if ((t & 63) == 0) {
#pragma unroll
        for (int q = 0; q < NV; ++q) sh[wave][q] = a[q];
    }
    __syncthreads();
    if (t < NV) {
        double s = sh[0][t];
#pragma unroll
        for (int w = 1; w < DIR_THREADS / 64; ++w) s += sh[w][t];
        total[t] = s;
    }
    __syncthreads();
}

// The adjoint of elastic_directional_kernel, one workgroup per crystal, a lane per direction in strides of DIR_THREADS.
// Nothing but the compliance is kept, so E(n) is made again per direction (by the forward's helpers: the same bits).
// With e = (1,1,1,0,0,0):  H = sum_d ( -gE_d E_d^2 v_d v_d^T + gbeta_d v_d e^T ),  g_compliance = (H + H^T) / 2.
// gE_d = the map's gradient plus the extremes' at the directions the forward recorded (a subgradient where values tie),
// gbeta_d likewise.  A lane accumulates the 21 distinct entries of the symmetric part and the 6 of sum_d gbeta_d v_d.
// Absent upstream gradients are skipped by workgroup-uniform branches; a row with flag bit 0 gets zeros, a direction
// whose E is not finite contributes nothing -- by a select, so a NaN from above does not reach the output.
__global__ void __launch_bounds__(DIR_THREADS) elastic_directional_bwd_kernel(
    const double* __restrict__ compliance, const int32_t* __restrict__ flags, const double* __restrict__ dirs, int n_dirs,
    const double* __restrict__ g_young, const double* __restrict__ g_beta, const double* __restrict__ g_ext,
    const int32_t* __restrict__ arg, double* __restrict__ g_compliance) {
    const int64_t b = blockIdx.x;
    const int t = threadIdx.x;
    double* out = g_compliance + b * 36;
    if (flags[b] & 1) {   // (uniform over the workgroup)
        if (t < 36) out[t] = 0.0;
        return;
    }
    double S[6][6];
    load_sym6(compliance + b * 36, S);
    int at[4] = {-1, -1, -1, -1};            // E_min, E_max, beta_min, beta_max: where, and their upstream gradients
    double gx[4] = {0.0, 0.0, 0.0, 0.0};
    if (g_ext) {
#pragma unroll
        for (int q = 0; q < 4; ++q) at[q] = arg[b * 4 + q], gx[q] = g_ext[b * 4 + q];
    }

    double acc[27];
#pragma unroll
    for (int q = 0; q < 27; ++q) acc[q] = 0.0;
    for (int d = t; d < n_dirs; d += DIR_THREADS) {
        double v[6], Sv[6];
        voigt_dyad(load_dir(dirs, d), v);
        matvec6(S, v, Sv);
        const double E = 1.0 / dot6(v, Sv);
        double gE = 0.0, gb = 0.0;
        if (g_young) gE = g_young[b * n_dirs + d];
        if (g_beta) gb = g_beta[b * n_dirs + d];
        gE += d == at[0] ? gx[0] : 0.0;
        gE += d == at[1] ? gx[1] : 0.0;
        gb += d == at[2] ? gx[2] : 0.0;
        gb += d == at[3] ? gx[3] : 0.0;
        const double a0 = -gE * (E * E);
        const double a = finite64(E) ? a0 : 0.0;
#pragma unroll
        for (int i = 0; i < 6; ++i) {
#pragma unroll
            for (int j = i; j < 6; ++j) acc[tri6(i, j)] += a * (v[i] * v[j]);
            acc[21 + i] += gb * v[i];
        }
    }
    __shared__ double total[27];
    block_sum<27>(acc, total, t);
    if (t < 36) {
        const int i = t / 6, j = t - 6 * i;
        const double sym = total[i <= j ? tri6(i, j) : tri6(j, i)];
        const double h_ij = sym + (j < 3 ? total[21 + i] : 0.0), h_ji = sym + (i < 3 ? total[21 + j] : 0.0);
        out[t] = 0.5 * (h_ij + h_ji);
    }
}

// The adjoint of elastic_acoustic_kernel, one workgroup per crystal, a lane per direction in strides of DIR_THREADS.
// Gamma and its Jacobi sweeps are run again (christoffel, sym3_eig) with the eigenvectors u_k; with s = modulus_unit / rho,
// v_k = sqrt(lambda_k s):
//   w_k = (g_vel_k + [slowest here] g_ext_0 + [fastest here] g_ext_1 - 3 g_ext_2 v_k^-4) s / (2 v_k),
//   Gbar = sum_k w_k u_k u_k^T,   Hc[V[i][j]][V[k][l]] += Gbar_ik n_j n_l  (symmetric: 21 distinct entries per lane),
//   g_voigt = (Hc + Hc^T) / 2 = Hc.
// Exactly degenerate modes: the per-mode terms take whatever orthonormal basis Jacobi left (finite, basis-dependent as
// the derivative itself is undefined); the sum_inv_v3 term weights the modes by one function of lambda and is
// basis-independent.  A row with flag bit 0 or a density that is not positive and finite gets zeros; a direction the
// forward marked unstable contributes nothing -- by a select on its whole contribution.
__global__ void __launch_bounds__(DIR_THREADS) elastic_acoustic_bwd_kernel(
    const double* __restrict__ voigt, const int32_t* __restrict__ flags, const double* __restrict__ density,
    const double* __restrict__ dirs, int n_dirs, double modulus_unit, const double* __restrict__ g_vel,
    const double* __restrict__ g_ext, const int32_t* __restrict__ arg, double* __restrict__ g_voigt) {
    const int64_t b = blockIdx.x;
    const int t = threadIdx.x;
    double* out = g_voigt + b * 36;
    const double rho = density[b];
    if ((flags[b] & 1) || !(rho > 0.0) || !finite64(rho)) {   // (uniform over the workgroup)
        if (t < 36) out[t] = 0.0;
        return;
    }
    double C[6][6];
    load_sym6(voigt + b * 36, C);
    const double scale = modulus_unit / rho;
    int at_slow = -1, at_fast = -1;
    double gx_slow = 0.0, gx_fast = 0.0, gx_sum = 0.0;
    if (g_ext) {
        at_slow = arg[b * 2 + 0], at_fast = arg[b * 2 + 1];
        gx_slow = g_ext[b * 3 + 0], gx_fast = g_ext[b * 3 + 1], gx_sum = g_ext[b * 3 + 2];
    }

    double acc[21];
#pragma unroll
    for (int q = 0; q < 21; ++q) acc[q] = 0.0;
    for (int d = t; d < n_dirs; d += DIR_THREADS) {
        const double n[3] = {dirs[d * 3 + 0], dirs[d * 3 + 1], dirs[d * 3 + 2]};
        double G[3][3], lam[3], U[3][3];   // column k of U = u_k
        christoffel(C, n, G);
        sym3_eig<true>(G, lam, U);
        const bool ok = stable3(lam);
        sort3(lam, U);
        double w[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double vk = sqrt(lam[k] * scale), v2 = vk * vk;
            double g = 0.0;
            if (g_vel) g = g_vel[(b * n_dirs + d) * 3 + k];
            if (k == 0) g += d == at_slow ? gx_slow : 0.0;
            if (k == 2) g += d == at_fast ? gx_fast : 0.0;
            w[k] = (g - 3.0 * gx_sum / (v2 * v2)) * (scale / (2.0 * vk));
        }
        double Gb[3][3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int k = i; k < 3; ++k)
                Gb[i][k] = Gb[k][i] = (w[0] * (U[i][0] * U[k][0]) + w[1] * (U[i][1] * U[k][1])) + w[2] * (U[i][2] * U[k][2]);
        }
        double h[21];
#pragma unroll
        for (int q = 0; q < 21; ++q) h[q] = 0.0;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int j = 0; j < 3; ++j) {
#pragma unroll
                for (int k = 0; k < 3; ++k) {
#pragma unroll
                    for (int l = 0; l < 3; ++l) {
                        if (VOIGT_OF[i][j] <= VOIGT_OF[k][l]) h[tri6(VOIGT_OF[i][j], VOIGT_OF[k][l])] += Gb[i][k] * (n[j] * n[l]);
                    }
                }
            }
        }
#pragma unroll
        for (int q = 0; q < 21; ++q) acc[q] += ok ? h[q] : 0.0;
    }
    __shared__ double total[21];
    block_sum<21>(acc, total, t);
    if (t < 36) {
        const int i = t / 6, j = t - 6 * i;
        out[t] = total[i <= j ? tri6(i, j) : tri6(j, i)];   // Hc is symmetric: (Hc + Hc^T) / 2 is Hc itself
    }
}

// ---------------------------------------------------------------------------------------------------
// refinement of the grid's extremes (elastic_properties(refine=True)): the winners of the directional and the pair kernel
// polished off the grid.  matten_amd/elastic.py:refine_extremes_host is the same iteration in numpy.
// ---------------------------------------------------------------------------------------------------
// (cross3, dot3, add3, scale3: csrc/elastic_dirs.h)

// A(a) x with the symmetric A(a) = [[2 a0, a5, a4], [a5, 2 a1, a3], [a4, a3, 2 a2]]: a . v(n) = n^T A(a) n / 2 and
// a . w(n,m) = n^T A(a) m, so A(a) x is the derivative of either
__device__ __forceinline__ V3 sym_apply(const double (&a)[6], V3 x) {
    return {2.0 * a[0] * x.x + a[5] * x.y + a[4] * x.z, a[5] * x.x + 2.0 * a[1] * x.y + a[3] * x.z,
            a[4] * x.x + a[3] * x.y + 2.0 * a[2] * x.z};
}

// kind 0: E(n), 1: G(n,m), 2: nu(n,m) (the definitions above elastic_pair_kernel) with df/dn and df/dm, n and m taken as
// independent vectors
__device__ __forceinline__ void refine_eval(int kind, const double (&S)[6][6], V3 n, V3 m, double& f, V3& dn, V3& dm) {
    if (kind == 1) {
        double w[6], Sw[6];
        voigt_pair(n, m, w);
        matvec6(S, w, Sw);
        f = 1.0 / dot6(w, Sw);
        const double c = -2.0 * f * f;
        dn = scale3(c, sym_apply(Sw, m));
        dm = scale3(c, sym_apply(Sw, n));
        return;
    }
    double v[6], Sv[6];
    voigt_dyad(n, v);
    matvec6(S, v, Sv);
    const double q = dot6(v, Sv);
    if (kind == 0) {
        f = 1.0 / q;
        dn = scale3(-2.0 * f * f, sym_apply(Sv, n));
        dm = {0.0, 0.0, 0.0};
        return;
    }
    double vm[6], Svm[6];
    voigt_dyad(m, vm);
    matvec6(S, vm, Svm);
    const double p = dot6(Sv, vm);
    f = -p / q;
    dn = add3(scale3(-1.0 / q, sym_apply(Svm, n)), scale3(2.0 * p / (q * q), sym_apply(Sv, n)));
    dm = scale3(-1.0 / q, sym_apply(Sv, m));
}

// F = sign f at the pair and its gradient over rotations of the pair, n x dF/dn + m x dF/dm
__device__ __forceinline__ void refine_grad(int kind, double sign, const double (&S)[6][6], V3 n, V3 m, double& F, V3& g) {
    double f;
    V3 dn, dm;
    refine_eval(kind, S, n, m, f, dn, dm);
    F = sign * f;
    g = scale3(sign, add3(cross3(n, dn), cross3(m, dm)));
}

// R(w) x = x + a (w x x) + b (w x (w x x)), a = sin|w| / |w|, b = (1 - cos|w|) / |w|^2 (Rodrigues)
__device__ __forceinline__ void rot_coeff(V3 w, double& a, double& b) {
    const double t2 = dot3(w, w), t = sqrt(t2), sh = sin(0.5 * t);
    const bool tiny = t2 < 1e-16;
    a = tiny ? 1.0 : sin(t) / t;
    b = tiny ? 0.5 : 2.0 * sh * sh / t2;
}
__device__ __forceinline__ V3 rot_apply(V3 w, double a, double b, V3 x) {
    const V3 wx = cross3(w, x);
    return add3(x, add3(scale3(a, wx), scale3(b, cross3(w, wx))));
}
__device__ __forceinline__ void orthonormal(V3& n, V3& m) {
    n = scale3(1.0 / sqrt(dot3(n, n)), n);
    m = add3(m, scale3(-dot3(m, n), n));
    m = scale3(1.0 / sqrt(dot3(m, m)), m);
}
// a column of the gradient's central differences: the rotation e (|e| = h, coefficients a, b) and its opposite
__device__ __forceinline__ V3 refine_fd(int kind, double sign, const double (&S)[6][6], V3 n, V3 m, V3 e, double a, double b,
                                        double inv_2h) {
    const V3 o = {-e.x, -e.y, -e.z};
    double F;
    V3 gp, gm;
    refine_grad(kind, sign, S, rot_apply(e, a, b, n), rot_apply(e, a, b, m), F, gp);
    refine_grad(kind, sign, S, rot_apply(o, a, b, n), rot_apply(o, a, b, m), F, gm);
    return {(gp.x - gm.x) * inv_2h, (gp.y - gm.y) * inv_2h, (gp.z - gm.z) * inv_2h};
}

// the iteration's constants (elastic.py holds the same, with the reasons)
constexpr double REFINE_FD_STEP = 6.103515625e-05;   // 2^-14 rad
constexpr double REFINE_MAX_STEP = 0.3;
constexpr double REFINE_CLAMP = 1e-3;
constexpr double REFINE_STALL_TOL = 1e-7;
constexpr int REFINE_DAMP_TRIES = 30;
constexpr int REFINE_THREADS = 64;

// One thread per (extreme q, crystal b), item = q n + b: a wave works on one kind of extreme (but for the one that holds a
// boundary).  q = 0..3: E_min, E_max, beta_min, beta_max from the directional kernel's ext / arg; 4..7: G_min, G_max,
// nu_min, nu_max from the pair kernel's.  The start pair is the winner's n with m = cos(chi_k) e1 + sin(chi_k) e2 in the
// pair kernel's frame (pair_frame, frame_dir; k = 0 for E and beta).  E, G, nu: F(w) = +-f(R(w) n, R(w) m) is maximised by a
// damped Newton iteration -- the analytic gradient at w = 0, the Hessian as the symmetric part of that gradient's central differences
// over rotations about the three axes, diagonalised by cyclic Jacobi, every eigenvalue clamped to the ascent side
// (min(lambda, -1e-3 max|lambda|), so directions the function does not depend on -- m for E, chi for G at a cubic [100] --
// and an isotropic tensor are harmless), the step capped at 0.3 rad, accepted only if the value strictly improves, else
// damped and tried again; the pair is made orthonormal again after every step.  beta = n^T B n: the extreme eigenvalues
// of B with their eigenvectors, no iteration.  No atomics, no cross-lane traffic, nothing read back: a row's result does
// not depend on the other rows and is bitwise reproducible.
__global__ void __launch_bounds__(REFINE_THREADS) elastic_refine_kernel(
    const double* __restrict__ compliance, const int32_t* __restrict__ flags, const double* __restrict__ dirs, int n_dirs,
    const double* __restrict__ cos_sin, int n_ang, const double* __restrict__ ext_dir, const int32_t* __restrict__ arg_dir,
    const double* __restrict__ ext_pair, const int32_t* __restrict__ arg_pair, int64_t n, int n_q, double tol, int max_iter,
    double* __restrict__ value, double* __restrict__ vec_n, double* __restrict__ vec_m, int32_t* __restrict__ status,
    int32_t* __restrict__ iterations) {
    const int64_t item = (int64_t)blockIdx.x * REFINE_THREADS + threadIdx.x;
    if (item >= n * n_q) return;
    const int q = (int)(item / n);
    const int64_t b = item - (int64_t)q * n;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    const bool pairq = q >= 4;
    const int fl = flags[b];
    const double grid = pairq ? ext_pair[b * 4 + (q - 4)] : ext_dir[b * 4 + q];
    const int at = pairq ? arg_pair[b * 4 + (q - 4)] : arg_dir[b * 4 + q];
    const int64_t n_start = pairq ? (int64_t)n_dirs * n_ang : (int64_t)n_dirs;

    double val = nan;
    V3 n_out = {nan, nan, nan}, m_out = {nan, nan, nan};
    int st = -1, it = 0;
    if (!(fl & 1) && at >= 0 && at < n_start) {   // (an index outside the tables is never followed)
        const int d = pairq ? at / n_ang : at, k = pairq ? at - d * n_ang : 0;
        const V3 n0 = load_dir(dirs, d);
        V3 e1, e2;
        pair_frame(n0, e1, e2);
        const V3 m0 = frame_dir(pairq ? cos_sin[2 * (int64_t)k] : 1.0, pairq ? cos_sin[2 * (int64_t)k + 1] : 0.0, e1, e2);
        const double sign = (q & 1) ? 1.0 : -1.0;
        // load_sym6, written out: through the helper the compiler orders this kernel's arithmetic differently, and at one
        // wave per SIMD that schedule took 0.15 ms where this one takes 0.11 (docs/LAB_NOTES.md).  The mean of two values
        // does not depend on their order, so S holds the other kernels' bits either way.
        const double* s = compliance + b * 36;
        double S[6][6];
#pragma unroll
        for (int i = 0; i < 6; ++i) {
#pragma unroll
            for (int j = i; j < 6; ++j) S[i][j] = S[j][i] = 0.5 * (s[i * 6 + j] + s[j * 6 + i]);
        }

        V3 nn = n0, mm = m0;
        if (fl & 2) {   // not positive definite: E and nu have poles, nothing is followed
            val = grid;
            st = 2;
        } else if (q == 2 || q == 3) {
            double r[6], A[3][3], lam[3], U[3][3];
            compress_rows(S, r);
            A[0][0] = r[0], A[1][1] = r[1], A[2][2] = r[2], A[0][1] = 0.5 * r[5], A[0][2] = 0.5 * r[4], A[1][2] = 0.5 * r[3];
            sym3_eig<true>(A, lam, U);
            sort3(lam, U);
            const bool top = q == 3;
            val = top ? lam[2] : lam[0];
            nn = top ? V3{U[0][2], U[1][2], U[2][2]} : V3{U[0][0], U[1][0], U[2][0]};
            mm = {U[0][1], U[1][1], U[2][1]};
            st = 0;
        } else {
            const int kind = q < 2 ? 0 : (q < 6 ? 1 : 2);
            double ah, bh;
            rot_coeff({REFINE_FD_STEP, 0.0, 0.0}, ah, bh);
            const double inv_2h = 1.0 / (2.0 * REFINE_FD_STEP);
            for (;;) {
                double F0;
                V3 g;
                refine_grad(kind, sign, S, nn, mm, F0, g);
                val = sign * F0;
                if (!finite64(F0)) {
                    val = grid;
                    st = 2;
                    break;
                }
                const double scale = kind == 2 ? fmax(fabs(F0), 1.0) : fabs(F0);
                const double gnorm = sqrt(dot3(g, g));
                if (gnorm <= tol * scale) {
                    st = 0;
                    break;
                }
                if (it >= max_iter) {
                    st = 1;
                    break;
                }
                const V3 d0 = refine_fd(kind, sign, S, nn, mm, {REFINE_FD_STEP, 0.0, 0.0}, ah, bh, inv_2h);
                const V3 d1 = refine_fd(kind, sign, S, nn, mm, {0.0, REFINE_FD_STEP, 0.0}, ah, bh, inv_2h);
                const V3 d2 = refine_fd(kind, sign, S, nn, mm, {0.0, 0.0, REFINE_FD_STEP}, ah, bh, inv_2h);
                // H_ij = (D_ij + D_ji) / 2, D_ij = d g_i / d w_j (column j = d_j)
                double A[3][3], lam[3], U[3][3];
                A[0][0] = d0.x, A[1][1] = d1.y, A[2][2] = d2.z;
                A[0][1] = 0.5 * (d1.x + d0.y), A[0][2] = 0.5 * (d2.x + d0.z), A[1][2] = 0.5 * (d2.y + d1.z);
                sym3_eig<true>(A, lam, U);
                const double dl = REFINE_CLAMP * fmax(fabs(lam[0]), fmax(fabs(lam[1]), fabs(lam[2]))) + 1e-300;
                const double l0 = fmin(lam[0], -dl), l1 = fmin(lam[1], -dl), l2 = fmin(lam[2], -dl);
                const double ug0 = U[0][0] * g.x + U[1][0] * g.y + U[2][0] * g.z,
                             ug1 = U[0][1] * g.x + U[1][1] * g.y + U[2][1] * g.z,
                             ug2 = U[0][2] * g.x + U[1][2] * g.y + U[2][2] * g.z;
                double damp = 0.0;
                bool moved = false;
                for (int tries = 0; tries < REFINE_DAMP_TRIES; ++tries) {
                    const double c0 = -ug0 / (l0 - damp), c1 = -ug1 / (l1 - damp), c2 = -ug2 / (l2 - damp);
                    V3 step = {U[0][0] * c0 + U[0][1] * c1 + U[0][2] * c2, U[1][0] * c0 + U[1][1] * c1 + U[1][2] * c2,
                               U[2][0] * c0 + U[2][1] * c1 + U[2][2] * c2};
                    const double len = sqrt(dot3(step, step));
                    step = len > REFINE_MAX_STEP ? scale3(REFINE_MAX_STEP / len, step) : step;
                    double ra, rb;
                    rot_coeff(step, ra, rb);
                    V3 n1 = rot_apply(step, ra, rb, nn), m1 = rot_apply(step, ra, rb, mm);
                    orthonormal(n1, m1);
                    double f1;
                    V3 unused_n, unused_m;
                    refine_eval(kind, S, n1, m1, f1, unused_n, unused_m);
                    if (sign * f1 > F0) {
                        nn = n1, mm = m1, moved = true;
                        break;
                    }
                    damp = fmax(2.0 * damp, dl);
                }
                if (!moved) {   // no step improves the value any more: stationary to fp64
                    st = gnorm <= fmax(tol, REFINE_STALL_TOL) * scale ? 0 : 1;
                    break;
                }
                ++it;
            }
        }
        // rounding alone can leave the result behind the grid's (a constant beta, an isotropic E); a NaN fails the
        // comparison too: the grid's value and pair then
        const bool keep = sign * val >= sign * grid;
        val = keep ? val : grid;
        n_out = keep ? nn : n0;
        m_out = keep ? mm : m0;
    }
    value[item] = val;
    vec_n[item * 3 + 0] = n_out.x, vec_n[item * 3 + 1] = n_out.y, vec_n[item * 3 + 2] = n_out.z;
    vec_m[item * 3 + 0] = m_out.x, vec_m[item * 3 + 1] = m_out.y, vec_m[item * 3 + 2] = m_out.z;
    status[item] = st;
    iterations[item] = it;
}

}  // namespace

extern "C" int matten_elastic_props(const void* c, int is_fp64, int layout, int64_t n, double* voigt, double* compliance,
                                    double* props, int32_t* flags, matten_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (n < 0 || (layout != 0 && layout != 1) || (is_fp64 != 0 && is_fp64 != 1)) return MATTEN_EINVAL;
    if (n == 0) return MATTEN_OK;
    if (!c || !voigt || !compliance || !props || !flags) return MATTEN_EINVAL;
    const int T = 64;
    const unsigned grid = (unsigned)matten_cdiv(n, T);
    if (is_fp64) {
        if (layout == 0) elastic_props_kernel<double, 0><<<grid, T, 0, stream>>>((const double*)c, n, voigt, compliance, props, flags);
        else elastic_props_kernel<double, 1><<<grid, T, 0, stream>>>((const double*)c, n, voigt, compliance, props, flags);
    } else {
        if (layout == 0) elastic_props_kernel<float, 0><<<grid, T, 0, stream>>>((const float*)c, n, voigt, compliance, props, flags);
        else elastic_props_kernel<float, 1><<<grid, T, 0, stream>>>((const float*)c, n, voigt, compliance, props, flags);
    }
    MATTEN_LAUNCH_CHECK();
    return MATTEN_OK;
}

extern "C" int matten_elastic_props_bwd(const double* voigt, const double* compliance, const double* props, const int32_t* flags,
                                        const double* g_props, const double* g_voigt, const double* g_compliance, int is_fp64,
                                        int layout, int64_t n, void* g_c, matten_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (n < 0 || (layout != 0 && layout != 1) || (is_fp64 != 0 && is_fp64 != 1)) return MATTEN_EINVAL;
    if (n == 0) return MATTEN_OK;
    if (!voigt || !compliance || !props || !flags || !g_props || !g_c) return MATTEN_EINVAL;
    const int T = 64;
    const unsigned grid = (unsigned)matten_cdiv(n, T);
#define BWD_(TYPE, LAYOUT) \
    elastic_props_bwd_kernel<TYPE, LAYOUT><<<grid, T, 0, stream>>>(compliance, props, flags, g_props, g_voigt, g_compliance, n, (TYPE*)g_c)
    if (is_fp64) {
        if (layout == 0) BWD_(double, 0);
        else BWD_(double, 1);
    } else {
        if (layout == 0) BWD_(float, 0);
        else BWD_(float, 1);
    }
#undef BWD_
    MATTEN_LAUNCH_CHECK();
    return MATTEN_OK;
}

// the sizes of a direction-set entry: n crystals (n_max bounds the kernel's 32-bit item count), n_dirs directions of three
// coordinates, n_angles angles per direction (1 where the entry has none), the pairs counted in 32 bits
static bool dir_set_ok(int64_t n, int64_t n_max, int64_t n_dirs, int64_t n_angles) {
    return n >= 0 && n <= n_max && n_dirs >= 1 && n_dirs <= 0x7fffffff / 3 && n_angles >= 0 && n_angles <= 0x7fffffff &&
           n_dirs * n_angles <= 0x7fffffff;
}

extern "C" int matten_elastic_directional(const double* compliance, const int32_t* flags, const double* dirs, int64_t n,
                                          int64_t n_dirs, double* young, double* beta, double* ext, int32_t* arg,
                                          matten_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!dir_set_ok(n, 0x7fffffff, n_dirs, 1)) return MATTEN_EINVAL;
    if (n == 0) return MATTEN_OK;
    if (!compliance || !flags || !dirs || !ext || !arg) return MATTEN_EINVAL;
    elastic_directional_kernel<<<(unsigned)n, DIR_THREADS, 0, stream>>>(compliance, flags, dirs, (int)n_dirs, young, beta, ext,
                                                                        arg);
    MATTEN_LAUNCH_CHECK();
    return MATTEN_OK;
}

extern "C" int matten_elastic_pair(const double* compliance, const int32_t* flags, const double* dirs, const double* cos_sin,
                                   int64_t n, int64_t n_dirs, int64_t n_angles, double* maps, double* ext, int32_t* arg,
                                   matten_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!dir_set_ok(n, 0x7fffffff, n_dirs, n_angles) || n_angles < 1) return MATTEN_EINVAL;
    if (n == 0) return MATTEN_OK;
    if (!compliance || !flags || !dirs || !cos_sin || !ext || !arg) return MATTEN_EINVAL;
    elastic_pair_kernel<<<(unsigned)n, DIR_THREADS, 0, stream>>>(compliance, flags, dirs, (int)n_dirs, cos_sin, (int)n_angles,
                                                                 maps, ext, arg);
    MATTEN_LAUNCH_CHECK();
    return MATTEN_OK;
}

extern "C" int matten_elastic_acoustic(const double* voigt, const int32_t* flags, const double* density, const double* dirs,
                                       int64_t n, int64_t n_dirs, double modulus_unit, double* vel, double* ext, int32_t* arg,
                                       int32_t* n_unstable, matten_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!dir_set_ok(n, 0x7fffffff, n_dirs, 1)) return MATTEN_EINVAL;
    if (n == 0) return MATTEN_OK;
    if (!voigt || !flags || !density || !dirs || !ext || !arg || !n_unstable) return MATTEN_EINVAL;
    elastic_acoustic_kernel<<<(unsigned)n, DIR_THREADS, 0, stream>>>(voigt, flags, density, dirs, (int)n_dirs, modulus_unit, vel,
                                                                     ext, arg, n_unstable);
    MATTEN_LAUNCH_CHECK();
    return MATTEN_OK;
}

extern "C" int matten_elastic_directional_bwd(const double* compliance, const int32_t* flags, const double* dirs, int64_t n,
                                              int64_t n_dirs, const double* g_young, const double* g_beta, const double* g_ext,
                                              const int32_t* arg, double* g_compliance, matten_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!dir_set_ok(n, 0x7fffffff, n_dirs, 1) || (g_ext && !arg)) return MATTEN_EINVAL;
    if (n == 0) return MATTEN_OK;
    if (!compliance || !flags || !dirs || !g_compliance) return MATTEN_EINVAL;
    elastic_directional_bwd_kernel<<<(unsigned)n, DIR_THREADS, 0, stream>>>(compliance, flags, dirs, (int)n_dirs, g_young, g_beta,
                                                                            g_ext, arg, g_compliance);
    MATTEN_LAUNCH_CHECK();
    return MATTEN_OK;
}

extern "C" int matten_elastic_acoustic_bwd(const double* voigt, const int32_t* flags, const double* density, const double* dirs,
                                           int64_t n, int64_t n_dirs, double modulus_unit, const double* g_vel,
                                           const double* g_ext, const int32_t* arg, double* g_voigt, matten_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!dir_set_ok(n, 0x7fffffff, n_dirs, 1) || (g_ext && !arg)) return MATTEN_EINVAL;
    if (n == 0) return MATTEN_OK;
    if (!voigt || !flags || !density || !dirs || !g_voigt) return MATTEN_EINVAL;
    elastic_acoustic_bwd_kernel<<<(unsigned)n, DIR_THREADS, 0, stream>>>(voigt, flags, density, dirs, (int)n_dirs, modulus_unit,
                                                                         g_vel, g_ext, arg, g_voigt);
    MATTEN_LAUNCH_CHECK();
    return MATTEN_OK;
}

extern "C" int matten_elastic_refine(const double* compliance, const int32_t* flags, const double* dirs, const double* cos_sin,
                                     const double* ext_dir, const int32_t* arg_dir, const double* ext_pair,
                                     const int32_t* arg_pair, int64_t n, int64_t n_dirs, int64_t n_angles, double tol,
                                     int64_t max_iter, double* value, double* vec_n, double* vec_m, int32_t* status,
                                     int32_t* iterations, matten_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!dir_set_ok(n, 0x7fffffff / 8, n_dirs, n_angles) || !(tol > 0.0) || !(tol <= 1.7976931348623157e308) || max_iter < 0 ||
        max_iter > 0x7fffffff)
        return MATTEN_EINVAL;
    if (n == 0) return MATTEN_OK;
    if (!compliance || !flags || !dirs || !ext_dir || !arg_dir || !value || !vec_n || !vec_m || !status || !iterations)
        return MATTEN_EINVAL;
    if (n_angles > 0 && (!cos_sin || !ext_pair || !arg_pair)) return MATTEN_EINVAL;
    const int n_q = n_angles > 0 ? 8 : 4;
    elastic_refine_kernel<<<(unsigned)matten_cdiv(n * n_q, REFINE_THREADS), REFINE_THREADS, 0, stream>>>(
        compliance, flags, dirs, (int)n_dirs, cos_sin, (int)n_angles, ext_dir, arg_dir, ext_pair, arg_pair, n, n_q, tol,
        (int)max_iter, value, vec_n, vec_m, status, iterations);
    MATTEN_LAUNCH_CHECK();
    return MATTEN_OK;
}
