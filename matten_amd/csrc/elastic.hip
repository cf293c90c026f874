// Derived elastic properties of predicted elasticity tensors (include/matten_hip.h, "Derived elastic properties").
//   elastic_props_kernel       : Voigt matrix, compliance, the ten scalar moduli and the flags   reference predict.py:217-218
//   elastic_directional_kernel : Young's modulus and linear compressibility over a direction set, with their extremes
// The reference wraps every predicted tensor in pymatgen's ElasticTensor (one Python object per crystal); these two kernels
// compute what its users read off that object.  All arithmetic is fp64; everything is held in registers with compile-time
// indices, so no kernel here uses scratch memory (hipcc -Rpass-analysis=kernel-resource-usage: DESIGN.md).
#include "common.h"

namespace {

// pymatgen's Voigt order xx, yy, zz, yz, xz, xy
__device__ constexpr int VI[6] = {0, 1, 2, 1, 0, 0};
__device__ constexpr int VJ[6] = {0, 1, 2, 2, 2, 1};

__device__ __forceinline__ constexpr int cart(int i, int j, int k, int l) { return ((i * 3 + j) * 3 + k) * 3 + l; }

__device__ __forceinline__ bool finite64(double v) { return fabs(v) <= 1.7976931348623157e308; }   // false for NaN

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
        const T* p = c + b * 36;
#pragma unroll
        for (int I = 0; I < 6; ++I) {
#pragma unroll
            for (int J = I; J < 6; ++J) C[I][J] = C[J][I] = 0.5 * ((double)p[I * 6 + J] + (double)p[J * 6 + I]);
        }
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

// (value, direction index) pairs ordered by value, equal values by the lower index: a total order, so the butterfly
// below gives every lane the same winner whatever the pairing -- bitwise reproducible
struct Ext {
    double v;
    int i;
};
template <bool MAX>
__device__ __forceinline__ Ext better(Ext a, Ext b) {
    const bool take_b = (MAX ? b.v > a.v : b.v < a.v) || (b.v == a.v && b.i < a.i);
    return take_b ? b : a;
}
template <bool MAX>
__device__ __forceinline__ Ext wave_best(Ext a) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        Ext o;
        o.v = __shfl_xor(a.v, off, 64);
        o.i = __shfl_xor(a.i, off, 64);
        a = better<MAX>(a, o);
    }
    return a;
}

constexpr int DIR_THREADS = 256;

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
    // the 21 distinct entries (the two triangles of the elimination's result agree to rounding: their mean), and the
    // row sums of the compressibility
    const double* s = compliance + b * 36;
    double S[6][6], r[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
#pragma unroll
        for (int j = i; j < 6; ++j) S[i][j] = S[j][i] = 0.5 * (s[i * 6 + j] + s[j * 6 + i]);
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) r[i] = S[i][0] + S[i][1] + S[i][2];

    const double inf = __longlong_as_double(0x7ff0000000000000LL);
    Ext e_min = {inf, 0x7fffffff}, e_max = {-inf, 0x7fffffff}, b_min = {inf, 0x7fffffff}, b_max = {-inf, 0x7fffffff};
    for (int d = t; d < n_dirs; d += DIR_THREADS) {
        const double n1 = dirs[d * 3 + 0], n2 = dirs[d * 3 + 1], n3 = dirs[d * 3 + 2];
        const double v[6] = {n1 * n1, n2 * n2, n3 * n3, n2 * n3, n1 * n3, n1 * n2};
        double q = 0.0, bt = 0.0;
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            double row = 0.0;
#pragma unroll
            for (int j = 0; j < 6; ++j) row += S[i][j] * v[j];
            q += v[i] * row;
            bt += r[i] * v[i];
        }
        const double E = 1.0 / q;
        if (young) young[b * n_dirs + d] = E;
        if (beta) beta[b * n_dirs + d] = bt;
        const Ext ce = {E, d}, cb = {bt, d};
        e_min = better<false>(e_min, ce);
        e_max = better<true>(e_max, ce);
        b_min = better<false>(b_min, cb);
        b_max = better<true>(b_max, cb);
    }
    // in the wave first, then across the four waves through LDS
    e_min = wave_best<false>(e_min);
    e_max = wave_best<true>(e_max);
    b_min = wave_best<false>(b_min);
    b_max = wave_best<true>(b_max);
    __shared__ double sh_v[DIR_THREADS / 64][4];
    __shared__ int sh_i[DIR_THREADS / 64][4];
    const int wave = t >> 6;
    if ((t & 63) == 0) {
        sh_v[wave][0] = e_min.v, sh_v[wave][1] = e_max.v, sh_v[wave][2] = b_min.v, sh_v[wave][3] = b_max.v;
        sh_i[wave][0] = e_min.i, sh_i[wave][1] = e_max.i, sh_i[wave][2] = b_min.i, sh_i[wave][3] = b_max.i;
    }
    __syncthreads();
    if (t < 4) {
        Ext a = {sh_v[0][t], sh_i[0][t]};
#pragma unroll
        for (int w = 1; w < DIR_THREADS / 64; ++w) {
            const Ext o = {sh_v[w][t], sh_i[w][t]};
            a = (t & 1) ? better<true>(a, o) : better<false>(a, o);
        }
        ext[b * 4 + t] = a.v;
        arg[b * 4 + t] = a.i;
    }
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

extern "C" int matten_elastic_directional(const double* compliance, const int32_t* flags, const double* dirs, int64_t n,
                                          int64_t n_dirs, double* young, double* beta, double* ext, int32_t* arg,
                                          matten_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (n < 0 || n_dirs < 1 || n_dirs > 0x7fffffff / 3 || n > 0x7fffffff) return MATTEN_EINVAL;
    if (n == 0) return MATTEN_OK;
    if (!compliance || !flags || !dirs || !ext || !arg) return MATTEN_EINVAL;
    elastic_directional_kernel<<<(unsigned)n, DIR_THREADS, 0, stream>>>(compliance, flags, dirs, (int)n_dirs, young, beta, ext,
                                                                        arg);
    MATTEN_LAUNCH_CHECK();
    return MATTEN_OK;
}
