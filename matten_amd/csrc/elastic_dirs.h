// What the direction-set kernels of csrc/elastic.hip (directional, pair, acoustic, their adjoints, the refinement) and of
// csrc/waves.hip (polarisations, group velocities, phonon focusing) share: the symmetrised Voigt matrix in registers, the
// frame of a direction, the Christoffel matrix, and the (value, index) extremes of a workgroup in a fixed order.  One copy:
// "the same frame" and "the same eigenvalues" between the two files is one piece of code.  fp64; every index is a
// compile-time constant, so nothing here goes to scratch memory.
#pragma once
#include "common.h"
#include "sym3.h"

namespace {

__device__ __forceinline__ bool finite64(double v) { return fabs(v) <= 1.7976931348623157e308; }   // false for NaN

struct V3 {
    double x, y, z;
};
__device__ __forceinline__ V3 load_dir(const double* __restrict__ dirs, int d) {
    return {dirs[d * 3 + 0], dirs[d * 3 + 1], dirs[d * 3 + 2]};
}
__device__ __forceinline__ V3 cross3(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ double dot3(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ V3 add3(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ V3 scale3(double c, V3 a) { return {c * a.x, c * a.y, c * a.z}; }

// a [36] Voigt matrix as the mean of its two triangles: the input is never trusted to be symmetric (the two triangles of
// the elimination's result agree to rounding only)
template <typename T>
__device__ __forceinline__ void load_sym6(const T* __restrict__ p, double (&M)[6][6]) {
#pragma unroll
    for (int i = 0; i < 6; ++i) {
#pragma unroll
        for (int j = i; j < 6; ++j) M[i][j] = M[j][i] = 0.5 * ((double)p[i * 6 + j] + (double)p[j * 6 + i]);
    }
}
__device__ __forceinline__ void matvec6(const double (&S)[6][6], const double (&x)[6], double (&y)[6]) {
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        double row = 0.0;
#pragma unroll
        for (int j = 0; j < 6; ++j) row += S[i][j] * x[j];
        y[i] = row;
    }
}

// the branch-free orthonormal frame (e1, e2) of a unit vector n: e1 x e2 = n
__device__ __forceinline__ void pair_frame(V3 n, V3& e1, V3& e2) {
    const double sg = n.z >= 0.0 ? 1.0 : -1.0;
    const double fa = -1.0 / (sg + n.z), fb = n.x * n.y * fa;
    e1 = {1.0 + sg * n.x * n.x * fa, sg * fb, -sg * n.x};
    e2 = {fb, sg + n.y * n.y * fa, -n.y};
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
constexpr int EXT_NONE = 0x7fffffff;   // the index of an Ext that no candidate has replaced yet

// the workgroup's winner of NV lane-local (value, index) pairs -- minima at even, maxima at odd positions -- written by lane
// q < NV to ext[q] / arg[q]: in the wave first, then across the four waves through LDS.  A pair that never met a comparable
// value (all NaN) becomes NaN and -1 with NONE_IS_NAN; without, it is written as it stands (+-inf and EXT_NONE: what the
// directional kernel has written since its first version)
template <int NV, bool NONE_IS_NAN>
__device__ __forceinline__ void block_best(Ext (&e)[NV], double* __restrict__ ext, int32_t* __restrict__ arg, int t) {
    __shared__ double sh_v[DIR_THREADS / 64][NV];
    __shared__ int sh_i[DIR_THREADS / 64][NV];
#pragma unroll
    for (int q = 0; q < NV; ++q) e[q] = (q & 1) ? wave_best<true>(e[q]) : wave_best<false>(e[q]);
    const int wave = t >> 6;
    if ((t & 63) == 0) {
#pragma unroll
        for (int q = 0; q < NV; ++q) sh_v[wave][q] = e[q].v, sh_i[wave][q] = e[q].i;
    }
    __syncthreads();
    if (t < NV) {
        Ext a = {sh_v[0][t], sh_i[0][t]};
#pragma unroll
        for (int w = 1; w < DIR_THREADS / 64; ++w) {
            const Ext o = {sh_v[w][t], sh_i[w][t]};
            a = (t & 1) ? better<true>(a, o) : better<false>(a, o);
        }
        const bool none = NONE_IS_NAN && a.i == EXT_NONE;
        ext[t] = none ? __longlong_as_double(0x7ff8000000000000LL) : a.v;
        arg[t] = none ? -1 : a.i;
    }
}

// Gamma_ik = C_ijkl n_j n_l, its upper triangle
__device__ constexpr int VOIGT_OF[3][3] = {{0, 5, 4}, {5, 1, 3}, {4, 3, 2}};   // Cartesian pair -> Voigt index
__device__ __forceinline__ void christoffel(const double (&C)[6][6], const double (&n)[3], double (&G)[3][3]) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int k = i; k < 3; ++k) {
            double g = 0.0;
#pragma unroll
            for (int j = 0; j < 3; ++j) {
#pragma unroll
                for (int l = 0; l < 3; ++l) g += C[VOIGT_OF[i][j]][VOIGT_OF[k][l]] * (n[j] * n[l]);
            }
            G[i][k] = g;
        }
    }
}

// (the cyclic Jacobi of a symmetric 3x3 matrix -- sym3_eig, sort3 -- is csrc/sym3.h)
// a direction is acoustically stable where all three eigenvalues of Gamma are positive and finite (false for NaN)
__device__ __forceinline__ bool stable3(const double (&lam)[3]) {
    return lam[0] > 0.0 && lam[1] > 0.0 && lam[2] > 0.0 && finite64(lam[0]) && finite64(lam[1]) && finite64(lam[2]);
}

}  // namespace
