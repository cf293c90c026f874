// Eigen-decomposition of a symmetric 6x6 matrix in registers by cyclic Jacobi: the 6x6 counterpart of csrc/sym3.h, used by
// csrc/kelvin.hip on the Mandel matrix of an elasticity tensor.  The rotation is sym3.h's (jacobi_rotate for the angle, the
// diagonal and the first of the four other rows, jacobi_turn for the rest): one copy.  fp64; the upper triangle is the
// matrix, every index is a compile-time constant, so nothing here goes to scratch memory.
#pragma once
#include "sym3.h"

namespace {

// Sweeps.  A numpy fp64 run of this exact rotation in this order over 869 Mandel matrices -- the 100 tensors of the example
// data set, isotropic and cubic tensors (K/G from 1e-5 to 3e5), random definite and indefinite matrices at entry scales 1e-3
// to 3e2, spectra graded over nine decades, orthogonally mixed 5-fold degenerate spectra -- leaves the largest off-diagonal
// entry, relative to max|C^|, at 1.1, 0.42, 0.15, 4.7e-3, 3.6e-8 after sweeps 1 to 5 and below 1e-20 after sweep 6 on every
// matrix but one: a mixed 5-fold degenerate one, 6.8e-19 = 0.003 eps, which later sweeps only halve -- rounding noise between
// diagonal entries that are equal to the last bit, inside an eigenspace where every basis is an eigenbasis.
// NEARLY degenerate moduli are what takes longest: a rotation inside a cluster split by s max|C^| starts to converge
// quadratically only once the off-diagonal is below s.  On 11 000 spectra [130,130,160,160,160,490], [80 x 5, 300],
// [100 x 3, 250 x 3] and [5 x 6] with relative splits of 1e-15 to 1e-3, mixed by random orthogonal 6x6 matrices, the
// worst off-diagonal is 7.3e-9, 1.5e-9 (a residual C^ U - U L of that size), 5.2e-13 after sweeps 6, 7, 8 and below
// 4.1e-19 after sweep 9 (the same rounding floor as above; at most 2 rows still above 1e-20).  Nine sweeps and one of
// margin; the eigenvalues are within 3.2e-15 max|C^| of LAPACK's from sweep 7 on.
constexpr int JACOBI6_SWEEPS = 10;

// the entry (I, J) of the symmetric matrix, which lives in the upper triangle
template <int I, int J>
__device__ __forceinline__ double& sym6_at(double (&A)[6][6]) {
    return A[I < J ? I : J][I < J ? J : I];
}
// the other four indices of the pair (P, Q), P < Q, ascending: K = 0..3
template <int P, int Q, int K>
struct sym6_other {
    static constexpr int lo = K + (K >= P ? 1 : 0);
    static constexpr int value = lo + (lo >= Q ? 1 : 0);
};

// One rotation: annihilates a_PQ.  The arithmetic on A does not depend on VEC.
template <bool VEC, int P, int Q>
__device__ __forceinline__ void jacobi6_step(double (&A)[6][6], double (&U)[6][6]) {
    constexpr int R0 = sym6_other<P, Q, 0>::value, R1 = sym6_other<P, Q, 1>::value, R2 = sym6_other<P, Q, 2>::value,
                  R3 = sym6_other<P, Q, 3>::value;
    double sn, tau;
    jacobi_rotate(A[P][P], A[Q][Q], A[P][Q], sym6_at<R0, P>(A), sym6_at<R0, Q>(A), sn, tau);
    jacobi_turn(sn, tau, sym6_at<R1, P>(A), sym6_at<R1, Q>(A));
    jacobi_turn(sn, tau, sym6_at<R2, P>(A), sym6_at<R2, Q>(A));
    jacobi_turn(sn, tau, sym6_at<R3, P>(A), sym6_at<R3, Q>(A));
    if (VEC) {
#pragma unroll
        for (int i = 0; i < 6; ++i) jacobi_turn(sn, tau, U[i][P], U[i][Q]);
    }
}
template <bool VEC, int P>
__device__ __forceinline__ void jacobi6_row(double (&A)[6][6], double (&U)[6][6]) {
    if constexpr (P + 1 < 6) jacobi6_step<VEC, P, P + 1>(A, U);
    if constexpr (P + 2 < 6) jacobi6_step<VEC, P, P + 2>(A, U);
    if constexpr (P + 3 < 6) jacobi6_step<VEC, P, P + 3>(A, U);
    if constexpr (P + 4 < 6) jacobi6_step<VEC, P, P + 4>(A, U);
    if constexpr (P + 5 < 6) jacobi6_step<VEC, P, P + 5>(A, U);
}

// The eigenvalues of the symmetric A (its upper triangle is read and destroyed) in lam, unsorted, by JACOBI6_SWEEPS cyclic
// sweeps in row order (0,1), (0,2), ... (4,5); with VEC the eigenvectors in the columns of U, which is not touched
// otherwise.  The sweeps are a loop, not unrolled (15 rotations of ~25 or ~50 fused multiply-adds each are the body); within
// one sweep every index is a constant.
template <bool VEC>
__device__ __forceinline__ void sym6_eig(double (&A)[6][6], double (&lam)[6], double (&U)[6][6]) {
    if (VEC) {
#pragma unroll
        for (int i = 0; i < 6; ++i) {
#pragma unroll
            for (int j = 0; j < 6; ++j) U[i][j] = i == j ? 1.0 : 0.0;
        }
    }
#pragma unroll 1
    for (int sweep = 0; sweep < JACOBI6_SWEEPS; ++sweep) {
        jacobi6_row<VEC, 0>(A, U);
        jacobi6_row<VEC, 1>(A, U);
        jacobi6_row<VEC, 2>(A, U);
        jacobi6_row<VEC, 3>(A, U);
        jacobi6_row<VEC, 4>(A, U);
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) lam[k] = A[k][k];
}

// (eigenvalue, eigenvector column) pairs in ascending order: the 12-comparator network for six keys (checked on all 64
// 0-1 inputs), exchanged by selects
template <bool VEC, int P, int Q>
__device__ __forceinline__ void sort6_pair(double (&lam)[6], double (&U)[6][6]) {
    const bool sw = lam[P] > lam[Q];
    const double a = lam[P], b = lam[Q];
    lam[P] = sw ? b : a, lam[Q] = sw ? a : b;
    if (VEC) {
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            const double x = U[i][P], y = U[i][Q];
            U[i][P] = sw ? y : x, U[i][Q] = sw ? x : y;
        }
    }
}
template <bool VEC>
__device__ __forceinline__ void sort6(double (&lam)[6], double (&U)[6][6]) {
    sort6_pair<VEC, 0, 5>(lam, U), sort6_pair<VEC, 1, 3>(lam, U), sort6_pair<VEC, 2, 4>(lam, U);
    sort6_pair<VEC, 1, 2>(lam, U), sort6_pair<VEC, 3, 4>(lam, U);
    sort6_pair<VEC, 0, 3>(lam, U), sort6_pair<VEC, 2, 5>(lam, U);
    sort6_pair<VEC, 0, 1>(lam, U), sort6_pair<VEC, 2, 3>(lam, U), sort6_pair<VEC, 4, 5>(lam, U);
    sort6_pair<VEC, 1, 2>(lam, U), sort6_pair<VEC, 3, 4>(lam, U);
}

}  // namespace
