// Textured polycrystals (include/matten_hip.h, "Textured polycrystals"): the Voigt, Reuss, Hill and geometric means of
// elasticity tensors under orientation distributions, as anisotropic aggregate tensors.
//   texture_slice_kernel / texture_finish_kernel : packed orientation lists -> one 21x21 operator per texture
//   texture_average_kernel                       : the four means of every aggregate, one aggregate per thread
//   texture_agg_bwd_kernel / texture_member_bwd_kernel / texture_crystal_sum_kernel : the adjoint
// The operator is what makes the cost of a texture independent of the number of crystals: <X> = sum_g w_g N_g X N_g^T is
// linear in the 21 upper-triangle entries of the symmetric Mandel matrix X, so G orientations collapse to 441 numbers once
// and every crystal pays one 21x21 product per mean.  fp64 throughout.  The averages work from the Kelvin decomposition
// that matten_elastic_kelvin wrote (S^ = U diag(1/l) U^T, L^ = U diag(log l) U^T); the two finishing steps -- the inverse
// of the mean compliance, the exponential of the mean logarithm -- are one sym6_eig each.  Every sum runs in a fixed order
// (orientations within a slice, slices, members, a crystal's memberships): no atomics, bitwise reproducible.
#include "common.h"
#include "sym6.h"

namespace {

constexpr int TX_THREADS = 64;            // aggregates, members or crystals per workgroup
constexpr int TX_OP = 441;                // entries of one operator
constexpr int TX_OP_THREADS = 448;        // seven waves: one thread per operator entry
constexpr int TX_BATCH = 64;              // orientations staged in LDS at a time
constexpr int TX_PART = 448;              // doubles per (texture, slice) partial: 441 sums, the weight sum, the bad flag
constexpr double TX_SQRT2 = 1.4142135623730951;      // fp64(sqrt 2)
constexpr double TX_RSQRT2 = 0.70710678118654757;    // fp64(1 / sqrt 2)

__device__ __forceinline__ bool tx_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }   // false for NaN
__device__ __forceinline__ constexpr double tx_mandel(int i, int j) {
    return (i < 3 && j < 3) ? 1.0 : ((i >= 3 && j >= 3) ? 2.0 : TX_SQRT2);
}
__device__ __forceinline__ constexpr double tx_unmandel(int i, int j) {
    return (i < 3 && j < 3) ? 1.0 : ((i >= 3 && j >= 3) ? 0.5 : TX_RSQRT2);
}
// the position of (i, j), i <= j, among the 21 upper-triangle entries in row-major order
__device__ __forceinline__ constexpr int tx_tri(int i, int j) { return i * 6 - i * (i - 1) / 2 + (j - i); }

// ---------------------------------------------------------------------------------------------------------------------
// the operator
// ---------------------------------------------------------------------------------------------------------------------
// N(R) = D Q(R) D^-1 (Q: Bond's matrix), row-major into n[36]; quadratic in R, so -R gives the same matrix.  Voigt pairs
// xx, yy, zz, yz, xz, xy.
__device__ __forceinline__ void tx_build_n(const double (&R)[3][3], double* n) {
    constexpr int pa[6] = {0, 1, 2, 1, 0, 0}, pb[6] = {0, 1, 2, 2, 2, 1};
#pragma unroll
    for (int I = 0; I < 6; ++I) {
#pragma unroll
        for (int J = 0; J < 6; ++J) {
            const int i = pa[I], j = pb[I], k = pa[J], l = pb[J];
            double v;
            if (I < 3 && J < 3) v = R[i][k] * R[i][k];
            else if (I < 3) v = TX_SQRT2 * (R[i][k] * R[i][l]);
            else if (J < 3) v = TX_SQRT2 * (R[i][k] * R[j][k]);
            else v = R[i][k] * R[j][l] + R[i][l] * R[j][k];
            n[I * 6 + J] = v;
        }
    }
}

// One workgroup per (texture, slice): the slice's orientations in order, 64 at a time through LDS; thread e owns the
// operator entry e = p * 21 + q.  part[(t * max_slices + s) * 448 + e]; slot 441 the weight sum, slot 442 the bad flag.
__global__ void __launch_bounds__(TX_OP_THREADS) texture_slice_kernel(const double* __restrict__ R, const double* __restrict__ weights,
                                                                      const int64_t* __restrict__ tex_ptr, int64_t G,
                                                                      int64_t slice_len, int64_t max_slices, double orth_tol,
                                                                      double* __restrict__ part) {
    __shared__ double sh_n[TX_BATCH][36];
    __shared__ double sh_w[TX_BATCH];
    const int64_t t = (int64_t)blockIdx.x / max_slices, s = (int64_t)blockIdx.x % max_slices;
    const int e = threadIdx.x;
    int64_t beg = tex_ptr[t], end = tex_ptr[t + 1];
    beg = beg < 0 ? 0 : beg;
    end = end > G ? G : end;
    if (s * slice_len >= end - beg) return;      // (the whole workgroup: this texture has fewer slices)
    const int64_t lo = beg + s * slice_len, hi = (end - lo > slice_len) ? lo + slice_len : end;

    // the four entries of N this thread multiplies: p = (I, J), q = (K, L)
    int I = 0, J = 0, K = 0, L = 0;
    {
        const int p = e < TX_OP ? e / 21 : 0, q = e < TX_OP ? e % 21 : 0;
        int c = 0;
        for (int i = 0; i < 6; ++i) {
            for (int j = i; j < 6; ++j, ++c) {
                if (c == p) I = i, J = j;
                if (c == q) K = i, L = j;
            }
        }
    }
    const int a0 = I * 6 + K, a1 = J * 6 + L, a2 = I * 6 + L, a3 = J * 6 + K;
    const double cross = K != L ? 1.0 : 0.0;

    double acc = 0.0, wsum = 0.0;
    int bad = 0;
    for (int64_t base = lo; base < hi; base += TX_BATCH) {
        const int nb = (int)((hi - base) < TX_BATCH ? (hi - base) : TX_BATCH);
        int mine = 0;
        if (e < nb) {
            double Rm[3][3];
            bool ok = true;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    Rm[i][j] = R[(base + e) * 9 + i * 3 + j];
                    ok = ok && tx_finite(Rm[i][j]);
                }
            }
            double skew = 0.0;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    const double d = (Rm[i][0] * Rm[j][0] + Rm[i][1] * Rm[j][1]) + Rm[i][2] * Rm[j][2] - (i == j ? 1.0 : 0.0);
                    skew = fmax(skew, fabs(d));
                }
            }
            const double w = weights ? weights[base + e] : 1.0;
            ok = ok && (skew <= orth_tol) && tx_finite(w) && (w >= 0.0);
            mine = ok ? 0 : 1;
            tx_build_n(Rm, sh_n[e]);
            sh_w[e] = w;
        }
        bad |= __syncthreads_or(mine);
        for (int g = 0; g < nb; ++g) {
            const double* n = sh_n[g];
            const double w = sh_w[g];
            acc += w * (n[a0] * n[a1] + cross * (n[a2] * n[a3]));
            wsum += w;
        }
        __syncthreads();
    }
    double* out = part + ((int64_t)blockIdx.x) * TX_PART;
    if (e < TX_OP) out[e] = acc;
    else if (e == TX_OP) out[e] = wsum;
    else if (e == TX_OP + 1) out[e] = bad ? 1.0 : 0.0;
}

// One workgroup per texture: the slices' partial sums added in slice order, divided by the weight sum.
__global__ void __launch_bounds__(TX_OP_THREADS) texture_finish_kernel(const int64_t* __restrict__ tex_ptr, int64_t G, int64_t slice_len,
                                                                       int64_t max_slices, const double* __restrict__ part,
                                                                       double* __restrict__ op, int32_t* __restrict__ tex_flags) {
    const int64_t t = blockIdx.x;
    const int e = threadIdx.x;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    int64_t beg = tex_ptr[t], end = tex_ptr[t + 1];
    beg = beg < 0 ? 0 : beg;
    end = end > G ? G : end;
    const int64_t len = end - beg;
    int64_t slices = len > 0 ? (len + slice_len - 1) / slice_len : 0;
    slices = slices > max_slices ? max_slices : slices;
    double acc = 0.0, wsum = 0.0;
    bool bad = slices == 0 || tex_ptr[t] < 0 || tex_ptr[t + 1] > G;
    for (int64_t s = 0; s < slices; ++s) {
        const double* p = part + (t * max_slices + s) * TX_PART;
        acc += e < TX_OP ? p[e] : 0.0;
        wsum += p[TX_OP];
        bad = bad || p[TX_OP + 1] != 0.0;
    }
    bad = bad || !(wsum > 0.0) || !tx_finite(wsum);
    if (e < TX_OP) op[t * TX_OP + e] = bad ? nan : acc / wsum;
    if (e == 0) tex_flags[t] = bad ? 1 : 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// shared pieces of the average and its adjoint
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool tx_load_decomposition(const double* __restrict__ moduli, const double* __restrict__ vectors,
                                                      int64_t c, double (&lam)[6], double (&U)[6][6]) {
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        lam[k] = moduli[c * 6 + k];
        ok = ok && tx_finite(lam[k]);
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) {
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            U[i][k] = vectors[c * 36 + i * 6 + k];
            ok = ok && tx_finite(U[i][k]);
        }
    }
    return ok;
}
// the upper triangle of U diag(w) U^T, k = 0..5 in order
__device__ __forceinline__ void tx_udu(const double (&U)[6][6], const double (&w)[6], double (&x)[21]) {
#pragma unroll
    for (int i = 0; i < 6; ++i) {
#pragma unroll
        for (int j = i; j < 6; ++j) {
            double acc = (U[i][0] * w[0]) * U[j][0];
#pragma unroll
            for (int k = 1; k < 6; ++k) acc += (U[i][k] * w[k]) * U[j][k];
            x[tx_tri(i, j)] = acc;
        }
    }
}
// the upper triangle of the Mandel matrix of a Voigt matrix (the mean of the two triangles, as kelvin.hip takes it)
__device__ __forceinline__ void tx_load_mandel(const double* __restrict__ p, double (&x)[21]) {
#pragma unroll
    for (int i = 0; i < 6; ++i) {
#pragma unroll
        for (int j = i; j < 6; ++j) x[tx_tri(i, j)] = tx_mandel(i, j) * (0.5 * (p[i * 6 + j] + p[j * 6 + i]));
    }
}
// P = U^T H U (upper triangle; H symmetric, given by its upper triangle)
__device__ __forceinline__ void tx_congruence_t(const double (&U)[6][6], const double (&h)[21], double (&P)[21]) {
    double T[6][6];      // T = H U
#pragma unroll
    for (int i = 0; i < 6; ++i) {
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            double acc = h[i <= 0 ? tx_tri(i, 0) : tx_tri(0, i)] * U[0][k];
#pragma unroll
            for (int j = 1; j < 6; ++j) acc += h[i <= j ? tx_tri(i, j) : tx_tri(j, i)] * U[j][k];
            T[i][k] = acc;
        }
    }
#pragma unroll
    for (int a = 0; a < 6; ++a) {
#pragma unroll
        for (int b = a; b < 6; ++b) {
            double acc = U[0][a] * T[0][b];
#pragma unroll
            for (int i = 1; i < 6; ++i) acc += U[i][a] * T[i][b];
            P[tx_tri(a, b)] = acc;
        }
    }
}
// X = U K U^T (upper triangle; K symmetric, given by its upper triangle)
__device__ __forceinline__ void tx_congruence(const double (&U)[6][6], const double (&k)[21], double (&X)[21]) {
    double T[6][6];      // T = K U^T
#pragma unroll
    for (int a = 0; a < 6; ++a) {
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            double acc = k[a <= 0 ? tx_tri(a, 0) : tx_tri(0, a)] * U[j][0];
#pragma unroll
            for (int b = 1; b < 6; ++b) acc += k[a <= b ? tx_tri(a, b) : tx_tri(b, a)] * U[j][b];
            T[a][j] = acc;
        }
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) {
#pragma unroll
        for (int j = i; j < 6; ++j) {
            double acc = U[i][0] * T[0][j];
#pragma unroll
            for (int a = 1; a < 6; ++a) acc += U[i][a] * T[a][j];
            X[tx_tri(i, j)] = acc;
        }
    }
}
// divided differences (f(a) - f(b)) / (a - b), finite where a == b
__device__ __forceinline__ double tx_dd_log(double a, double b) {
    const double t = (a - b) / b;
    return fabs(t) < 1e-6 ? (1.0 - t * 0.5 + t * t / 3.0) / b : log1p(t) / (t * b);
}
__device__ __forceinline__ double tx_dd_exp(double a, double b) {
    const double d = a - b;
    return exp(b) * (fabs(d) < 1e-6 ? 1.0 + d * 0.5 + d * d / 6.0 : expm1(d) / d);
}

// The state of an aggregate from its member list: -1, 2 or 0 (header), and the fraction sum.  Reads nothing through an
// index it has not checked.
__device__ __forceinline__ int tx_aggregate_state(const int32_t* __restrict__ flags, const double* __restrict__ moduli,
                                                  const double* __restrict__ vectors, int64_t n,
                                                  const int32_t* __restrict__ tex_flags, int64_t T,
                                                  const int32_t* __restrict__ member_crystal,
                                                  const int32_t* __restrict__ member_texture,
                                                  const double* __restrict__ member_fraction, int64_t lo, int64_t hi, double& fsum) {
    bool ok = hi > lo, pd = true;
    fsum = 0.0;
#pragma unroll 1
    for (int64_t m = lo; m < hi; ++m) {
        const int64_t c = member_crystal[m], t = member_texture[m];
        const double f = member_fraction[m];
        ok = ok && tx_finite(f) && f >= 0.0;
        fsum += f;
        if (c < 0 || c >= n || t < 0 || t >= T) {
            ok = false;
            continue;
        }
        double lam[6], U[6][6];
        const int fl = flags[c];
        ok = tx_load_decomposition(moduli, vectors, c, lam, U) && ok;
        ok = ok && (fl & 1) == 0 && tex_flags[t] == 0;
        pd = pd && (fl & 2) == 0 && lam[0] > 0.0;
    }
    ok = ok && fsum > 0.0 && tx_finite(fsum);
    return !ok ? -1 : (pd ? 0 : 2);
}

// ---------------------------------------------------------------------------------------------------------------------
// the four means: one aggregate per thread
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void tx_store_voigt(double* __restrict__ o, const double (&x)[21], bool ok) {
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
#pragma unroll
    for (int i = 0; i < 6; ++i) {
#pragma unroll
        for (int j = i; j < 6; ++j) {
            const double v = ok ? tx_unmandel(i, j) * x[tx_tri(i, j)] : nan;
            o[i * 6 + j] = v;
            if (j != i) o[j * 6 + i] = v;
        }
    }
}

__global__ void __launch_bounds__(TX_THREADS) texture_average_kernel(
    const double* __restrict__ voigt, const int32_t* __restrict__ flags, const double* __restrict__ moduli,
    const double* __restrict__ vectors, int64_t n, const double* __restrict__ op, const int32_t* __restrict__ tex_flags, int64_t T,
    const int32_t* __restrict__ member_crystal, const int32_t* __restrict__ member_texture,
    const double* __restrict__ member_fraction, int64_t M, const int64_t* __restrict__ agg_ptr, int64_t A, double* __restrict__ out,
    int32_t* __restrict__ status) {
    const int64_t a = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= A) return;
    int64_t lo = agg_ptr[a], hi = agg_ptr[a + 1];
    const bool range = lo >= 0 && hi <= M && lo <= hi;
    if (!range) lo = hi = 0;
    double fsum;
    const int st = tx_aggregate_state(flags, moduli, vectors, n, tex_flags, T, member_crystal, member_texture, member_fraction,
                                      lo, hi, fsum);
    status[a] = st;
    double* o = out + a * 144;
    double xv[21];      // the Voigt mean, kept for Hill's
    if (st == -1) {
#pragma unroll
        for (int q = 0; q < 21; ++q) xv[q] = 0.0;
#pragma unroll 1
        for (int k = 0; k < 4; ++k) tx_store_voigt(o + k * 36, xv, false);
        return;
    }
    // kind 0: C^ itself; 1: S^ = U diag(1/l) U^T, finished by an inverse; 2: L^ = U diag(log l) U^T, finished by exp
#pragma unroll 1
    for (int kind = 0; kind < 3; ++kind) {
        if (kind > 0 && st != 0) {
            tx_store_voigt(o + (kind == 1 ? 1 : 3) * 36, xv, false);
            if (kind == 1) tx_store_voigt(o + 2 * 36, xv, false);
            continue;
        }
        double acc[21];
#pragma unroll
        for (int q = 0; q < 21; ++q) acc[q] = 0.0;
#pragma unroll 1
        for (int64_t m = lo; m < hi; ++m) {
            const int64_t c = member_crystal[m];
            const double* __restrict__ P = op + (int64_t)member_texture[m] * TX_OP;
            const double f = member_fraction[m] / fsum;
            double x[21];
            if (kind == 0) {
                tx_load_mandel(voigt + c * 36, x);
            } else {
                double lam[6], U[6][6], w[6];
                tx_load_decomposition(moduli, vectors, c, lam, U);
#pragma unroll
                for (int k = 0; k < 6; ++k) w[k] = kind == 1 ? 1.0 / lam[k] : log(lam[k]);
                tx_udu(U, w, x);
            }
#pragma unroll
            for (int p = 0; p < 21; ++p) {
                double r = P[p * 21] * x[0];
#pragma unroll
                for (int q = 1; q < 21; ++q) r += P[p * 21 + q] * x[q];
                acc[p] += f * r;
            }
        }
        if (kind == 0) {
#pragma unroll
            for (int q = 0; q < 21; ++q) xv[q] = acc[q];
            tx_store_voigt(o, xv, true);
            continue;
        }
        double Am[6][6], lam[6], W[6][6], w[6], x[21];
#pragma unroll
        for (int i = 0; i < 6; ++i) {
#pragma unroll
            for (int j = i; j < 6; ++j) Am[i][j] = acc[tx_tri(i, j)];
        }
        sym6_eig<true>(Am, lam, W);
#pragma unroll
        for (int k = 0; k < 6; ++k) w[k] = kind == 1 ? 1.0 / lam[k] : exp(lam[k]);
        tx_udu(W, w, x);
        tx_store_voigt(o + (kind == 1 ? 1 : 3) * 36, x, true);
        if (kind == 1) {
#pragma unroll
            for (int q = 0; q < 21; ++q) x[q] = 0.5 * (xv[q] + x[q]);
            tx_store_voigt(o + 2 * 36, x, true);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// the adjoint
// ---------------------------------------------------------------------------------------------------------------------
// the gradient with respect to the symmetric Mandel matrix behind one of the four Voigt outputs, upper triangle
__device__ __forceinline__ void tx_load_gradient(const double* __restrict__ g, bool live, double scale, double (&x)[21], bool add) {
#pragma unroll
    for (int i = 0; i < 6; ++i) {
#pragma unroll
        for (int j = i; j < 6; ++j) {
            const double v = live ? scale * (tx_unmandel(i, j) * (0.5 * (g[i * 6 + j] + g[j * 6 + i]))) : 0.0;
            x[tx_tri(i, j)] = add ? x[tx_tri(i, j)] + v : v;
        }
    }
}

// Per aggregate: the gradients with respect to the three averaged matrices (mean C^, mean S^, mean L^), as gradients with
// respect to their 21 independent entries (off-diagonal entries doubled), so that the members apply the plain transpose
// of their operator.  agg_work [A,64]: 21 + 21 + 21, then the fraction sum.
__global__ void __launch_bounds__(TX_THREADS) texture_agg_bwd_kernel(const double* __restrict__ member_fraction, int64_t M,
                                                                     const int64_t* __restrict__ agg_ptr, int64_t A,
                                                                     const double* __restrict__ out, const int32_t* __restrict__ status,
                                                                     const double* __restrict__ g_out, double* __restrict__ agg_work) {
    const int64_t a = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= A) return;
    const int st = status[a];
    const bool all = st == 0, some = st == 0 || st == 2;
    const double* g = g_out + a * 144;
    const double* o = out + a * 144;
    double* w = agg_work + a * 64;

    int64_t lo = agg_ptr[a], hi = agg_ptr[a + 1];
    if (!(lo >= 0 && hi <= M && lo <= hi)) lo = hi = 0;
    double fsum = 0.0;
#pragma unroll 1
    for (int64_t m = lo; m < hi; ++m) fsum += member_fraction[m];
    w[63] = fsum;

    double x[21];
    // mean C^: voigt's, half of hill's
    tx_load_gradient(g, some, 1.0, x, false);
    tx_load_gradient(g + 72, all, 0.5, x, true);
#pragma unroll
    for (int i = 0; i < 6; ++i) {
#pragma unroll
        for (int j = i; j < 6; ++j) w[tx_tri(i, j)] = (i == j ? 1.0 : 2.0) * x[tx_tri(i, j)];
    }
    // mean S^: g = -C_R (g_reuss + g_hill / 2) C_R, with C_R the Reuss mean the forward wrote
    {
        tx_load_gradient(g + 36, all, 1.0, x, false);
        tx_load_gradient(g + 72, all, 0.5, x, true);
        double cr[21], T[6][6];
        tx_load_mandel(o + 36, cr);
#pragma unroll
        for (int i = 0; i < 6; ++i) {      // T = G C_R
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                double acc = 0.0;
#pragma unroll
                for (int j = 0; j < 6; ++j)
                    acc += x[i <= j ? tx_tri(i, j) : tx_tri(j, i)] * cr[j <= k ? tx_tri(j, k) : tx_tri(k, j)];
                T[i][k] = acc;
            }
        }
#pragma unroll
        for (int i = 0; i < 6; ++i) {
#pragma unroll
            for (int j = i; j < 6; ++j) {
                double acc = 0.0;
#pragma unroll
                for (int k = 0; k < 6; ++k) acc += cr[i <= k ? tx_tri(i, k) : tx_tri(k, i)] * T[k][j];
                const double v = -(i == j ? 1.0 : 2.0) * acc;
                w[21 + tx_tri(i, j)] = all && tx_finite(v) ? v : 0.0;
            }
        }
    }
    // mean L^: Daleckii-Krein for exp at the mean logarithm, whose eigenvectors are those of the geometric mean itself
    {
        double geo[21], Am[6][6], gam[6], W[6][6], P[21], X[21];
        tx_load_mandel(o + 108, geo);
#pragma unroll
        for (int i = 0; i < 6; ++i) {
#pragma unroll
            for (int j = i; j < 6; ++j) Am[i][j] = all ? geo[tx_tri(i, j)] : (i == j ? 1.0 : 0.0);
        }
        sym6_eig<true>(Am, gam, W);
        tx_load_gradient(g + 108, all, 1.0, x, false);
        tx_congruence_t(W, x, P);
#pragma unroll
        for (int i = 0; i < 6; ++i) {
#pragma unroll
            for (int j = i; j < 6; ++j) P[tx_tri(i, j)] *= tx_dd_exp(log(gam[i]), log(gam[j]));
        }
        tx_congruence(W, P, X);
#pragma unroll
        for (int i = 0; i < 6; ++i) {
#pragma unroll
            for (int j = i; j < 6; ++j) {
                const double v = (i == j ? 1.0 : 2.0) * X[tx_tri(i, j)];
                w[42 + tx_tri(i, j)] = all && tx_finite(v) ? v : 0.0;
            }
        }
    }
}

// Per member: rows [M,21] = the member's contribution to the gradient of its crystal's C^ (symmetric, upper triangle).
__global__ void __launch_bounds__(TX_THREADS) texture_member_bwd_kernel(
    const double* __restrict__ moduli, const double* __restrict__ vectors, const double* __restrict__ op,
    const int32_t* __restrict__ member_crystal, const int32_t* __restrict__ member_texture,
    const double* __restrict__ member_fraction, int64_t M, const int64_t* __restrict__ agg_ptr, int64_t A,
    const int32_t* __restrict__ status, const double* __restrict__ agg_work, double* __restrict__ rows) {
    const int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= M) return;
    double* r = rows + m * 21;
    // the aggregate of member m: the last a with agg_ptr[a] <= m
    int64_t a0 = 0, a1 = A;
    while (a1 - a0 > 1) {
        const int64_t mid = (a0 + a1) >> 1;
        if (agg_ptr[mid] <= m) a0 = mid;
        else a1 = mid;
    }
    const int64_t a = a0;
    const bool inside = agg_ptr[a] <= m && m < agg_ptr[a + 1];
    const int st = inside ? status[a] : -1;
    if (!(st == 0 || st == 2)) {      // (no index of this member was checked by the forward: none is used)
#pragma unroll
        for (int q = 0; q < 21; ++q) r[q] = 0.0;
        return;
    }
    const int64_t c = member_crystal[m];
    const double* __restrict__ P = op + (int64_t)member_texture[m] * TX_OP;
    const double* w = agg_work + a * 64;
    const double f = member_fraction[m] / w[63];
    const bool all = st == 0;

    // h = op^T g for the three averaged matrices at once (mean C^, mean S^, mean L^): each operator entry is read once,
    // rows p in order; an aggregate with status 2 has zeros for the last two
    double hv[21], hs[21], hl[21];
#pragma unroll
    for (int q = 0; q < 21; ++q) hv[q] = hs[q] = hl[q] = 0.0;
#pragma unroll 1
    for (int p = 0; p < 21; ++p) {
        const double gv = w[p], gs = w[21 + p], gl = w[42 + p];
#pragma unroll
        for (int q = 0; q < 21; ++q) {
            const double o = P[p * 21 + q];
            hv[q] += o * gv;
            hs[q] += o * gs;
            hl[q] += o * gl;
        }
    }
    // back to the entries of a symmetric matrix, with the member's fraction
#pragma unroll
    for (int i = 0; i < 6; ++i) {
#pragma unroll
        for (int j = i; j < 6; ++j) {
            const double s = i == j ? f : 0.5 * f;
            hv[tx_tri(i, j)] *= s, hs[tx_tri(i, j)] *= s, hl[tx_tri(i, j)] *= s;
        }
    }
    // through 1/x and through log, in the eigenbasis of C^
    double lam[6], U[6][6], Ksum[21], Pm[21];
    tx_load_decomposition(moduli, vectors, c, lam, U);
    tx_congruence_t(U, hs, Pm);
#pragma unroll
    for (int i = 0; i < 6; ++i) {
#pragma unroll
        for (int j = i; j < 6; ++j) Ksum[tx_tri(i, j)] = -Pm[tx_tri(i, j)] / (lam[i] * lam[j]);
    }
    tx_congruence_t(U, hl, Pm);
#pragma unroll
    for (int i = 0; i < 6; ++i) {
#pragma unroll
        for (int j = i; j < 6; ++j) Ksum[tx_tri(i, j)] += tx_dd_log(lam[i], lam[j]) * Pm[tx_tri(i, j)];
    }
    double X[21];
    tx_congruence(U, Ksum, X);
#pragma unroll
    for (int q = 0; q < 21; ++q) {
        const double v = hv[q] + (all ? X[q] : 0.0);
        r[q] = tx_finite(v) ? v : 0.0;
    }
}

// Per crystal: its members' rows added in member order (crystal_ptr / crystal_member: the members of each crystal,
// ascending), g_voigt = D g_C^ D, every element written.
__global__ void __launch_bounds__(TX_THREADS) texture_crystal_sum_kernel(const int64_t* __restrict__ crystal_ptr,
                                                                         const int32_t* __restrict__ crystal_member, int64_t n,
                                                                         int64_t M, const double* __restrict__ rows,
                                                                         double* __restrict__ g_voigt) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n) return;
    int64_t lo = crystal_ptr[c], hi = crystal_ptr[c + 1];
    if (!(lo >= 0 && hi <= M && lo <= hi)) lo = hi = 0;
    double acc[21];
#pragma unroll
    for (int q = 0; q < 21; ++q) acc[q] = 0.0;
#pragma unroll 1
    for (int64_t k = lo; k < hi; ++k) {
        const int64_t m = crystal_member[k];
        if (m < 0 || m >= M) continue;
#pragma unroll
        for (int q = 0; q < 21; ++q) acc[q] += rows[m * 21 + q];
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) {
#pragma unroll
        for (int j = i; j < 6; ++j) {
            const double v = tx_mandel(i, j) * acc[tx_tri(i, j)];
            g_voigt[c * 36 + i * 6 + j] = v;
            if (j != i) g_voigt[c * 36 + j * 6 + i] = v;
        }
    }
}

}  // namespace

static bool texture_count_ok(int64_t n) { return n >= 0 && n <= (int64_t)0x7fffffff * TX_THREADS; }

extern "C" int matten_texture_operator(const double* R, const double* weights, const int64_t* tex_ptr, int64_t G, int64_t T,
                                       double orth_tol, int64_t slice_len, double* workspace, int64_t workspace_doubles,
                                       double* op, int32_t* tex_flags, matten_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (G < 0 || T < 0 || T > 0x7fffffff || slice_len < 1 || !(orth_tol >= 0.0) || !(orth_tol <= 1.7976931348623157e308))
        return MATTEN_EINVAL;
    if (T == 0) return MATTEN_OK;
    if (!tex_ptr || !op || !tex_flags || (G > 0 && !R)) return MATTEN_EINVAL;
    const int64_t max_slices = matten_cdiv(G, slice_len);
    if (max_slices > 0 && T > (int64_t)0x7fffffff / max_slices) return MATTEN_EINVAL;
    if (max_slices > 0 && (!workspace || workspace_doubles < T * max_slices * TX_PART)) return MATTEN_ENOMEM;
    if (max_slices > 0) {
        texture_slice_kernel<<<(unsigned)(T * max_slices), TX_OP_THREADS, 0, stream>>>(R, weights, tex_ptr, G, slice_len, max_slices,
                                                                                      orth_tol, workspace);
        MATTEN_LAUNCH_CHECK();
    }
    texture_finish_kernel<<<(unsigned)T, TX_OP_THREADS, 0, stream>>>(tex_ptr, G, slice_len, max_slices, workspace, op, tex_flags);
    MATTEN_LAUNCH_CHECK();
    return MATTEN_OK;
}

extern "C" int matten_texture_average(const double* voigt, const int32_t* flags, const double* moduli, const double* vectors,
                                      int64_t n, const double* op, const int32_t* tex_flags, int64_t T,
                                      const int32_t* member_crystal, const int32_t* member_texture, const double* member_fraction,
                                      int64_t M, const int64_t* agg_ptr, int64_t A, double* out, int32_t* status,
                                      matten_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!texture_count_ok(n) || !texture_count_ok(A) || !texture_count_ok(M) || T < 0 || T > 0x7fffffff) return MATTEN_EINVAL;
    if (A == 0) return MATTEN_OK;
    if (!agg_ptr || !out || !status) return MATTEN_EINVAL;
    if (M > 0 && (!member_crystal || !member_texture || !member_fraction)) return MATTEN_EINVAL;
    if (n > 0 && (!voigt || !flags || !moduli || !vectors)) return MATTEN_EINVAL;
    if (T > 0 && (!op || !tex_flags)) return MATTEN_EINVAL;
    texture_average_kernel<<<(unsigned)matten_cdiv(A, TX_THREADS), TX_THREADS, 0, stream>>>(
        voigt, flags, moduli, vectors, n, op, tex_flags, T, member_crystal, member_texture, member_fraction, M, agg_ptr, A, out, status);
    MATTEN_LAUNCH_CHECK();
    return MATTEN_OK;
}

extern "C" int matten_texture_average_bwd(const double* moduli, const double* vectors, int64_t n, const double* op, int64_t T,
                                          const int32_t* member_crystal, const int32_t* member_texture,
                                          const double* member_fraction, int64_t M, const int64_t* agg_ptr, int64_t A,
                                          const double* out, const int32_t* status, const double* g_out,
                                          const int64_t* crystal_ptr, const int32_t* crystal_member, double* workspace,
                                          int64_t workspace_doubles, double* g_voigt, matten_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!texture_count_ok(n) || !texture_count_ok(A) || !texture_count_ok(M) || T < 0 || T > 0x7fffffff) return MATTEN_EINVAL;
    if (n == 0) return MATTEN_OK;
    if (!crystal_ptr || !g_voigt || (M > 0 && !crystal_member)) return MATTEN_EINVAL;
    if (A > 0 && (!agg_ptr || !out || !status || !g_out)) return MATTEN_EINVAL;
    if (M > 0 && (!member_crystal || !member_texture || !member_fraction || !moduli || !vectors || !op || A == 0)) return MATTEN_EINVAL;
    if (A * 64 + M * 21 > 0 && (!workspace || workspace_doubles < A * 64 + M * 21)) return MATTEN_ENOMEM;
    double* agg_work = workspace;
    double* rows = workspace + A * 64;
    if (A > 0) {
        texture_agg_bwd_kernel<<<(unsigned)matten_cdiv(A, TX_THREADS), TX_THREADS, 0, stream>>>(member_fraction, M, agg_ptr, A, out,
                                                                                               status, g_out, agg_work);
        MATTEN_LAUNCH_CHECK();
    }
    if (M > 0) {
        texture_member_bwd_kernel<<<(unsigned)matten_cdiv(M, TX_THREADS), TX_THREADS, 0, stream>>>(
            moduli, vectors, op, member_crystal, member_texture, member_fraction, M, agg_ptr, A, status, agg_work, rows);
        MATTEN_LAUNCH_CHECK();
    }
    texture_crystal_sum_kernel<<<(unsigned)matten_cdiv(n, TX_THREADS), TX_THREADS, 0, stream>>>(crystal_ptr, crystal_member, n, M, rows,
                                                                                               g_voigt);
    MATTEN_LAUNCH_CHECK();
    return MATTEN_OK;
}
