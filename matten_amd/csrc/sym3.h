// Eigen-decomposition of a symmetric 3x3 matrix in registers by cyclic Jacobi, shared by csrc/elastic.hip (Christoffel
// matrices, the compressibility matrix, the refinement's Hessians) and csrc/rank2.hip (per-atom rank-2 tensors): one copy
// of the rotation.  fp64; every index is a compile-time constant, so nothing here goes to scratch memory.
#pragma once
#include "common.h"

namespace {

// a pair (g, f) of row or column entries p, q turned by the rotation (sn, tau)
__device__ __forceinline__ void jacobi_turn(double sn, double tau, double& g, double& f) {
    const double g0 = g, f0 = f;
    g = g0 - sn * (f0 + g0 * tau);
    f = f0 + sn * (g0 - f0 * tau);
}
// One cyclic-Jacobi rotation of a symmetric 3x3 matrix: annihilates a_pq; r is the third index.  Branch-free: a zero
// a_pq (where theta is inf or 0/0) rotates by nothing.  Hands back (sn, tau) for the eigenvectors.
__device__ __forceinline__ void jacobi_rotate(double& app, double& aqq, double& apq, double& arp, double& arq, double& sn,
                                              double& tau) {
    const double theta = (aqq - app) / (2.0 * apq);
    double tn = copysign(1.0, theta) / (fabs(theta) + sqrt(theta * theta + 1.0));   // (theta^2 = inf: 0)
    tn = apq == 0.0 ? 0.0 : tn;
    const double c = 1.0 / sqrt(tn * tn + 1.0);
    sn = tn * c, tau = sn / (1.0 + c);
    const double h = tn * apq;
    app -= h;
    aqq += h;
    apq = 0.0;
    jacobi_turn(sn, tau, arp, arq);
}

// cyclic Jacobi converges quadratically: on the example data set, isotropic and cubic tensors the off-diagonal is below
// 1e-21 max|C| after 4 sweeps (numpy fp64 run of this rotation); one more sweep is the margin
constexpr int JACOBI_SWEEPS = 5;

// The eigenvalues of the symmetric A (its upper triangle is read and destroyed) in lam, unsorted, by JACOBI_SWEEPS cyclic
// sweeps; with VEC the eigenvectors in the columns of U, which is not touched otherwise.  The arithmetic on the matrix does
// not depend on VEC: an adjoint that asks for the vectors gets the forward's eigenvalues, bit for bit.
template <bool VEC, int P, int Q>
__device__ __forceinline__ void jacobi_step(double (&A)[3][3], double (&U)[3][3]) {
    constexpr int R = 3 - P - Q;
    double sn, tau;
    jacobi_rotate(A[P][P], A[Q][Q], A[P][Q], A[R < P ? R : P][R < P ? P : R], A[R < Q ? R : Q][R < Q ? Q : R], sn, tau);
    if (VEC) {
#pragma unroll
        for (int i = 0; i < 3; ++i) jacobi_turn(sn, tau, U[i][P], U[i][Q]);
    }
}
template <bool VEC>
__device__ __forceinline__ void sym3_eig(double (&A)[3][3], double (&lam)[3], double (&U)[3][3]) {
    if (VEC) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int j = 0; j < 3; ++j) U[i][j] = i == j ? 1.0 : 0.0;
        }
    }
#pragma unroll
    for (int sweep = 0; sweep < JACOBI_SWEEPS; ++sweep) {
        jacobi_step<VEC, 0, 1>(A, U);
        jacobi_step<VEC, 0, 2>(A, U);
        jacobi_step<VEC, 1, 2>(A, U);
    }
    lam[0] = A[0][0], lam[1] = A[1][1], lam[2] = A[2][2];
}
// (eigenvalue, eigenvector column) pairs in ascending order: a network of three comparators, exchanged by selects
template <int P, int Q>
__device__ __forceinline__ void sort_pair(double (&lam)[3], double (&U)[3][3]) {
    const bool sw = lam[P] > lam[Q];
    const double a = lam[P], b = lam[Q];
    lam[P] = sw ? b : a, lam[Q] = sw ? a : b;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double x = U[i][P], y = U[i][Q];
        U[i][P] = sw ? y : x, U[i][Q] = sw ? x : y;
    }
}
__device__ __forceinline__ void sort3(double (&lam)[3], double (&U)[3][3]) {
    sort_pair<0, 1>(lam, U);
    sort_pair<1, 2>(lam, U);
    sort_pair<0, 1>(lam, U);
}

}  // namespace
