// Kelvin (eigen-stiffness) decomposition of elasticity tensors (include/matten_hip.h, "Kelvin moduli and mechanical
// stability"): the eigen-decomposition of the 6x6 Mandel matrix C^ = D C D, D = diag(1,1,1,sqrt2,sqrt2,sqrt2), of the
// symmetrised Voigt matrix that matten_elastic_props writes.
//   kelvin_kernel       : the six Kelvin moduli, ascending, their eigenvectors and the dilatation of each mode
//   kelvin_bwd_kernel   : the adjoint of the moduli, from the vectors the forward wrote (Jacobi is not run again)
//   kelvin_clamp_kernel : the Frobenius-nearest tensor whose Kelvin moduli are all >= floor, as a Voigt matrix
// The reference hands back ElasticTensor(t) (predict.py:217-218) and its users diagonalise per crystal on the host.  One
// crystal per thread, fp64, everything in registers (csrc/sym6.h): 21 doubles of the upper triangle and, with vectors, 36
// of U, all indexed by compile-time constants, so no kernel uses scratch memory (hipcc -Rpass-analysis=kernel-resource-usage;
// the numbers are in docs/LAB_NOTES.md).  A row is 48-624 bytes each way: no LDS, no tuning.
#include "common.h"
#include "sym6.h"

namespace {

constexpr int KV_THREADS = 64;
constexpr double KV_SQRT2 = 1.4142135623730951;      // fp64(sqrt 2)
constexpr double KV_RSQRT2 = 0.70710678118654757;    // fp64(1 / sqrt 2)

__device__ __forceinline__ bool kv_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }   // false for NaN

// the Mandel factor d_I d_J as a constant: 1, sqrt2 or exactly 2 (never sqrt2 * sqrt2), and its inverse
__device__ __forceinline__ constexpr double kv_mandel(int i, int j) {
    return (i < 3 && j < 3) ? 1.0 : ((i >= 3 && j >= 3) ? 2.0 : KV_SQRT2);
}
__device__ __forceinline__ constexpr double kv_unmandel(int i, int j) {
    return (i < 3 && j < 3) ? 1.0 : ((i >= 3 && j >= 3) ? 0.5 : KV_RSQRT2);
}

// VEC: with eigenvectors (vectors and / or dilatation are wanted); the moduli are the same bits either way (sym6.h).
// A row with flag bit 0, or with an entry of C^ that is not finite (the mean of the two triangles or the factor 2 can
// overflow where the input did not), is NaN in every output.
template <bool VEC>
__global__ void __launch_bounds__(KV_THREADS) kelvin_kernel(const double* __restrict__ voigt, const int32_t* __restrict__ flags,
                                                            int64_t n, double* __restrict__ moduli,
                                                            double* __restrict__ vectors, double* __restrict__ dilatation) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n) return;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);

    const double* p = voigt + b * 36;
    double A[6][6], lam[6], U[6][6];
    bool ok = (flags[b] & 1) == 0;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
#pragma unroll
        for (int j = i; j < 6; ++j) {
            A[i][j] = kv_mandel(i, j) * (0.5 * (p[i * 6 + j] + p[j * 6 + i]));   // the input is never trusted to be symmetric
            ok = ok && kv_finite(A[i][j]);
        }
    }
    sym6_eig<VEC>(A, lam, U);
    sort6<VEC>(lam, U);

#pragma unroll
    for (int k = 0; k < 6; ++k) moduli[b * 6 + k] = ok ? lam[k] : nan;
    if (VEC) {
        if (vectors) {
#pragma unroll
            for (int i = 0; i < 6; ++i) {
#pragma unroll
                for (int k = 0; k < 6; ++k) vectors[b * 36 + i * 6 + k] = ok ? U[i][k] : nan;
            }
        }
        if (dilatation) {   // (tr eps_k)^2 / 3: the trace of the eigenstrain is the sum of the three normal components
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                const double tr = (U[0][k] + U[1][k]) + U[2][k];
                dilatation[b * 6 + k] = ok ? tr * tr / 3.0 : nan;
            }
        }
    }
}

// sum_k U_ik w_k U_jk in the fixed order k = 0..5
__device__ __forceinline__ double kv_udu(const double (&U)[6][6], const double (&w)[6], int i, int j) {
    double acc = (U[i][0] * w[0]) * U[j][0];
#pragma unroll
    for (int k = 1; k < 6; ++k) acc += (U[i][k] * w[k]) * U[j][k];
    return acc;
}
__device__ __forceinline__ bool kv_load_vectors(const double* __restrict__ p, double (&U)[6][6]) {
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            U[i][k] = p[i * 6 + k];
            ok = ok && kv_finite(U[i][k]);
        }
    }
    return ok;
}

// g_C^ = U diag(g_moduli) U^T, g_voigt = D g_C^ D: symmetric, so the transpose of the forward's symmetrisation is the
// identity on it.  A row with flag bit 0, or whose vectors the forward wrote as NaN, gets exact zeros by a select: a NaN
// is never multiplied away.
__global__ void __launch_bounds__(KV_THREADS) kelvin_bwd_kernel(const double* __restrict__ vectors,
                                                                const int32_t* __restrict__ flags,
                                                                const double* __restrict__ g_moduli, int64_t n,
                                                                double* __restrict__ g_voigt) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n) return;
    double U[6][6], w[6];
    const bool ok = kv_load_vectors(vectors + b * 36, U) && (flags[b] & 1) == 0;
#pragma unroll
    for (int k = 0; k < 6; ++k) w[k] = g_moduli[b * 6 + k];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
#pragma unroll
        for (int j = i; j < 6; ++j) {
            const double g = kv_mandel(i, j) * kv_udu(U, w, i, j);
            const double out = ok ? g : 0.0;
            g_voigt[b * 36 + i * 6 + j] = out;
            if (j != i) g_voigt[b * 36 + j * 6 + i] = out;
        }
    }
}

// C+ = D^-1 U diag(max(lambda_k, floor)) U^T D^-1.  A row whose moduli are all >= floor reproduces its input bit for bit:
// its 36 entries of `voigt` are copied through a select, the reconstruction is not used for it (U Lambda U^T would return
// the input only to the residual of the decomposition).  A NaN modulus compares false both ways: such a row is not copied,
// the clamp keeps the NaN (a select, not fmax), and every entry of the row comes out NaN.
__global__ void __launch_bounds__(KV_THREADS) kelvin_clamp_kernel(const double* __restrict__ voigt,
                                                                  const double* __restrict__ moduli,
                                                                  const double* __restrict__ vectors, double floor, int64_t n,
                                                                  double* __restrict__ out) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n) return;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    double U[6][6], w[6];
    const bool finite = kv_load_vectors(vectors + b * 36, U);
    bool keep = true;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const double l = moduli[b * 6 + k];
        keep = keep && (l >= floor);
        w[k] = l < floor ? floor : l;
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) {
#pragma unroll
        for (int j = i; j < 6; ++j) {
            const double c = finite ? kv_unmandel(i, j) * kv_udu(U, w, i, j) : nan;
            out[b * 36 + i * 6 + j] = keep ? voigt[b * 36 + i * 6 + j] : c;
            if (j != i) out[b * 36 + j * 6 + i] = keep ? voigt[b * 36 + j * 6 + i] : c;
        }
    }
}

}  // namespace

static bool kelvin_n_ok(int64_t n) { return n >= 0 && n <= (int64_t)0x7fffffff * KV_THREADS; }

extern "C" int matten_elastic_kelvin(const double* voigt, const int32_t* flags, int64_t n, double* moduli, double* vectors,
                                     double* dilatation, matten_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!kelvin_n_ok(n)) return MATTEN_EINVAL;
    if (n == 0) return MATTEN_OK;
    if (!voigt || !flags || !moduli) return MATTEN_EINVAL;
    const unsigned grid = (unsigned)matten_cdiv(n, KV_THREADS);
    if (vectors || dilatation) kelvin_kernel<true><<<grid, KV_THREADS, 0, stream>>>(voigt, flags, n, moduli, vectors, dilatation);
    else kelvin_kernel<false><<<grid, KV_THREADS, 0, stream>>>(voigt, flags, n, moduli, nullptr, nullptr);
    MATTEN_LAUNCH_CHECK();
    return MATTEN_OK;
}

extern "C" int matten_elastic_kelvin_bwd(const double* vectors, const int32_t* flags, const double* g_moduli, int64_t n,
                                         double* g_voigt, matten_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!kelvin_n_ok(n)) return MATTEN_EINVAL;
    if (n == 0) return MATTEN_OK;
    if (!vectors || !flags || !g_moduli || !g_voigt) return MATTEN_EINVAL;
    const unsigned grid = (unsigned)matten_cdiv(n, KV_THREADS);
    kelvin_bwd_kernel<<<grid, KV_THREADS, 0, stream>>>(vectors, flags, g_moduli, n, g_voigt);
    MATTEN_LAUNCH_CHECK();
    return MATTEN_OK;
}

extern "C" int matten_elastic_kelvin_clamp(const double* voigt, const double* moduli, const double* vectors, double floor,
                                           int64_t n, double* out, matten_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!kelvin_n_ok(n) || !(floor >= 0.0) || !(floor <= 1.7976931348623157e308)) return MATTEN_EINVAL;
    if (n == 0) return MATTEN_OK;
    if (!voigt || !moduli || !vectors || !out) return MATTEN_EINVAL;
    const unsigned grid = (unsigned)matten_cdiv(n, KV_THREADS);
    kelvin_clamp_kernel<<<grid, KV_THREADS, 0, stream>>>(voigt, moduli, vectors, floor, n, out);
    MATTEN_LAUNCH_CHECK();
    return MATTEN_OK;
}
