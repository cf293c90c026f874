// Derived quantities of per-atom rank-2 tensors (include/matten_hip.h, "Derived quantities of per-atom rank-2 tensors").
//   rank2_props_kernel     : principal values and axes of the symmetrised tensor, isotropic value, span, skew and the
//                            Haeberlen reduced anisotropy and asymmetry, with the flags
//   rank2_props_bwd_kernel : its adjoint, from what the forward wrote (the input is not kept, Jacobi is not run again)
// The reference returns per-atom tensors as they are (predict.py:117-148, one 3x3 array per atom); NMR users read these
// scalars off them.  One atom per thread, fp64 arithmetic on (T + T^T)/2, everything in registers: the ascending order
// (csrc/sym3.h) and the Haeberlen order are selects on compile-time indices, so neither kernel uses scratch memory
// (hipcc -Rpass-analysis=kernel-resource-usage).  A row is 72-150 bytes each way: no LDS, no tuning.
#include "common.h"
#include "sym3.h"

namespace {

constexpr int R2_THREADS = 256;

__device__ __forceinline__ bool r2_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }   // false for NaN

template <typename T>
__global__ void __launch_bounds__(R2_THREADS) rank2_props_kernel(const T* __restrict__ t, int64_t n, double* __restrict__ vals,
                                                                 double* __restrict__ axes, double* __restrict__ props,
                                                                 int32_t* __restrict__ flags) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n) return;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);

    double in[3][3];
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            in[i][j] = (double)t[b * 9 + i * 3 + j];
            ok = ok && r2_finite(in[i][j]);
        }
    }
    // the symmetrised tensor: the input is never trusted to be symmetric (sym3_eig reads the upper triangle)
    double A[3][3], lam[3], U[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = i; j < 3; ++j) A[i][j] = A[j][i] = 0.5 * (in[i][j] + in[j][i]);
    }
    // the isotropic part comes off first, t = tr(A)/3 as rounded (A_ii - t is exact where the two are within a factor of
    // two): the axes are those of the deviator, and Jacobi on it resolves them to eps span / gap, not eps |A| / gap -- a
    // shielding tensor is a few hundred ppm of isotropic part under an anisotropy that can be a thousand times smaller.
    // Span, skew, zeta and eta are formed from the deviator's values d_k; l_k = t + d_k and iso = t + mean(d).
    const double t0 = ((A[0][0] + A[1][1]) + A[2][2]) / 3.0;
    A[0][0] -= t0, A[1][1] -= t0, A[2][2] -= t0;
    sym3_eig<true>(A, lam, U);
    sort3(lam, U);

    const double dev = ((lam[0] + lam[1]) + lam[2]) / 3.0;   // (the rounding residue of the deviator's trace)
    const double iso = t0 + dev;
    const double span = lam[2] - lam[0];
    const bool flat = ok && span == 0.0;                     // a multiple of the identity: skew = eta = 0 by definition
    const double skew = flat ? 0.0 : 3.0 * (lam[1] - dev) / span;
    // Haeberlen order: z the principal value furthest from iso (l3 when skew <= 0, ties included), y = 2, x the other extreme
    const bool z_hi = skew <= 0.0;
    const double lz = z_hi ? lam[2] : lam[0], lx = z_hi ? lam[0] : lam[2];
    const double zeta = lz - dev;
    const double eta = flat ? 0.0 : (lam[1] - lx) / zeta;
#pragma unroll
    for (int k = 0; k < 3; ++k) lam[k] += t0;

#pragma unroll
    for (int k = 0; k < 3; ++k) vals[b * 3 + k] = ok ? lam[k] : nan;
    if (axes) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int k = 0; k < 3; ++k) axes[b * 9 + i * 3 + k] = ok ? U[i][k] : nan;
        }
    }
    double* p = props + b * 5;
    p[0] = ok ? iso : nan, p[1] = ok ? span : nan, p[2] = ok ? skew : nan, p[3] = ok ? zeta : nan, p[4] = ok ? eta : nan;
    flags[b] = (ok ? 0 : 1) | (flat ? 2 : 0);
}

// w_k = g_vals_k + sum_q g_props_q dq/dl_k, g_T = U diag(w) U^T (symmetric: the symmetrisation's transpose is the identity
// on it).  Excluded terms are replaced by selects, never multiplied away.
template <typename T>
__global__ void __launch_bounds__(R2_THREADS) rank2_props_bwd_kernel(const double* __restrict__ axes,
                                                                     const double* __restrict__ props,
                                                                     const int32_t* __restrict__ flags,
                                                                     const double* __restrict__ g_vals,
                                                                     const double* __restrict__ g_props, int64_t n,
                                                                     T* __restrict__ g_t) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n) return;
    const int32_t f = flags[b];
    const bool bad = (f & 1) != 0, flat = (f & 2) != 0;

    double U[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int k = 0; k < 3; ++k) U[i][k] = axes[b * 9 + i * 3 + k];
    }
    const double span = props[b * 5 + 1], skew = props[b * 5 + 2], zeta = props[b * 5 + 3], eta = props[b * 5 + 4];

    double w[3] = {0.0, 0.0, 0.0};
    if (g_vals) {
#pragma unroll
        for (int k = 0; k < 3; ++k) w[k] = g_vals[b * 3 + k];
    }
    if (g_props) {
        const double g_iso = g_props[b * 5 + 0], g_span = g_props[b * 5 + 1], g_skew = g_props[b * 5 + 2];
        const double g_zeta = g_props[b * 5 + 3], g_eta = g_props[b * 5 + 4];
        const double third = 1.0 / 3.0;
        const bool z_hi = skew <= 0.0;
        // d zeta / d l = e_z - 1/3, e_z on l3 (z_hi) or l1; e_y - e_x = e_2 - e_1 (z_hi) or e_2 - e_3
        const double dz[3] = {(z_hi ? 0.0 : 1.0) - third, -third, (z_hi ? 1.0 : 0.0) - third};
        const double dyx[3] = {z_hi ? -1.0 : 0.0, 1.0, z_hi ? 0.0 : -1.0};
        const double dskew[3] = {(skew - 1.0) / span, 2.0 / span, (-skew - 1.0) / span};
        const double ds[3] = {-1.0, 0.0, 1.0};
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double deta = dyx[k] / zeta - (eta / zeta) * dz[k];
            double acc = w[k] + g_iso * third + g_span * ds[k] + g_zeta * dz[k];
            acc += flat ? 0.0 : g_skew * dskew[k] + g_eta * deta;      // a multiple of the identity: skew = eta = 0 identically
            w[k] = acc;
        }
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = i; j < 3; ++j) {
            const double g = (U[i][0] * w[0]) * U[j][0] + (U[i][1] * w[1]) * U[j][1] + (U[i][2] * w[2]) * U[j][2];
            const T out = (T)(bad ? 0.0 : g);
            g_t[b * 9 + i * 3 + j] = out;
            if (j != i) g_t[b * 9 + j * 3 + i] = out;
        }
    }
}

}  // namespace

static bool rank2_n_ok(int64_t n) { return n >= 0 && n <= (int64_t)0x7fffffff * R2_THREADS; }

extern "C" int matten_rank2_props(const void* t, int is_fp64, int64_t n, double* vals, double* axes, double* props,
                                  int32_t* flags, matten_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!rank2_n_ok(n) || (is_fp64 != 0 && is_fp64 != 1)) return MATTEN_EINVAL;
    if (n == 0) return MATTEN_OK;
    if (!t || !vals || !props || !flags) return MATTEN_EINVAL;
    const unsigned grid = (unsigned)matten_cdiv(n, R2_THREADS);
    if (is_fp64) rank2_props_kernel<double><<<grid, R2_THREADS, 0, stream>>>((const double*)t, n, vals, axes, props, flags);
    else rank2_props_kernel<float><<<grid, R2_THREADS, 0, stream>>>((const float*)t, n, vals, axes, props, flags);
    MATTEN_LAUNCH_CHECK();
    return MATTEN_OK;
}

extern "C" int matten_rank2_props_bwd(const double* vals, const double* axes, const double* props, const int32_t* flags,
                                      const double* g_vals, const double* g_props, int is_fp64, int64_t n, void* g_t,
                                      matten_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!rank2_n_ok(n) || (is_fp64 != 0 && is_fp64 != 1)) return MATTEN_EINVAL;
    if (n == 0) return MATTEN_OK;
    if (!vals || !axes || !props || !flags || !g_t) return MATTEN_EINVAL;
    const unsigned grid = (unsigned)matten_cdiv(n, R2_THREADS);
    if (is_fp64) rank2_props_bwd_kernel<double><<<grid, R2_THREADS, 0, stream>>>(axes, props, flags, g_vals, g_props, n, (double*)g_t);
    else rank2_props_bwd_kernel<float><<<grid, R2_THREADS, 0, stream>>>(axes, props, flags, g_vals, g_props, n, (float*)g_t);
    MATTEN_LAUNCH_CHECK();
    return MATTEN_OK;
}
