// Rotations and symmetry averages of irreps rows (include/matten_hip.h, "Rotations and symmetry of irreps tensors").
//   rot_wigner_kernel    : the real Wigner-D blocks D^0..D^lmax of the proper part det(M) M of each 3x3 matrix, with flags
//   rot_rotate_kernel    : out[r] = D(M_index[r]) x[r] (or D^T), one irrep copy of one row per thread
//   rot_average_kernel   : out[r] = sum_j w_j D(M_op_idx[j]) x[r] / sum_j w_j over the row's list of operations
//   rot_deviation_kernel : |x[r] - out[r]| / |x[r]| per row
//   rot_average_atoms_kernel : out[k] = mean_g D(R_{b,g}) x[src[g,k]]: per-atom rows over their crystal's operations, sources
//                          gathered through the atom permutation of csrc/spacegroup.hip
// The reference rotates in the Cartesian basis on the host (tests/model/test_tfn_tensor.py:98-139, a rank-4 einsum after
// utils.py:110-133 to_cartesian); here the rows stay in the irreps basis on the device.
// D^l comes from the harmonics themselves: Y_l(R p_k) = D^l Y_l(p_k) over 2l+1 fixed unit vectors p_k, so
// D^l = B^T W with B[k][i] = Y_l,i(R p_k) and W = (A^-1)^T, A[k][i] = Y_l,i(p_k), inverted on the host in fp64.  The points
// are the best-conditioned of 400 random sets (condition numbers in the tables below).  The harmonics are sh.h's closed
// forms restated in fp64 (sh.h is float-only).  fp64 arithmetic, every index a compile-time constant: no kernel uses
// scratch memory (hipcc -Rpass-analysis=kernel-resource-usage).  No atomics, sums in list order: bitwise reproducible.
#include "common.h"

namespace {

constexpr int ROT_THREADS = 128;
constexpr int ROT_MAX_K = 16;      // layout rows per call (they travel as a kernel argument)
constexpr int ROT_STRIDE = 165;    // doubles per rotation: 1 + 9 + 25 + 49 + 81

__host__ __device__ constexpr int rot_block_offset(int l) { return l * (4 * l * l - 1) / 3; }   // 0, 1, 10, 35, 84

template <int L> struct RotTab;
template <> struct RotTab<1> {   // condition number 1.25
    static constexpr double P[3][3] = {
        {-0.46712751346937137, -0.16115156884169282, -0.8693802723893518},
        {-0.768714793263941, 0.21621830474963946, 0.6019362186381283},
        {-0.00024430411431756245, 0.9646517443158537, -0.26352789701259427},
    };
    static constexpr double W[3][3] = {
        {-0.37751670264548076, -0.12002416869701814, -0.43900207955755827},
        {-0.5216694052943117, 0.07275683641950421, 0.2668121893055013},
        {0.05386095641601247, 0.5621477693591904, -0.1331418865517421},
    };
};
template <> struct RotTab<2> {   // condition number 2.22
    static constexpr double P[5][3] = {
        {-0.8213192801650885, 0.3798466393268155, -0.4256185741027113},
        {-0.6958587540397383, -0.517126512758455, -0.49835806828879825},
        {-0.09526451023855446, 0.9456900766856865, 0.31079728433052417},
        {-0.9806598047662398, 0.02056252038816895, 0.19463691857180232},
        {-0.07129911263174338, 0.4636106376056806, 0.883165677116576},
    };
    static constexpr double W[5][5] = {
        {0.3286228707850172, -0.39459001963882134, -0.08356970740808864, 0.06010335823026487, -0.06588760043322126},
        {0.263790262746867, 0.306115371861475, -0.017206297681802363, 0.16525069537008039, -0.1101979702492532},
        {-0.01809761396749537, -0.18233927229105462, 0.3550028361066905, 0.2643019318440752, -0.20385471267016858},
        {-0.2619687123791839, -0.0666440995982471, -0.14847545433854334, 0.25116054778268737, -0.3529737611646131},
        {-0.020726664053750562, -0.21693768372924352, -0.2755531211766717, 0.358143506519002, 0.193131617086908},
    };
};
template <> struct RotTab<3> {   // condition number 3.35
    static constexpr double P[7][3] = {
        {-0.8198468121296292, -0.5722656010145707, 0.019060077028083076},
        {-0.41781366363672806, -0.30427704848188536, 0.8560649626316962},
        {-0.03787407731383776, -0.45497623492988587, 0.8896978025805452},
        {-0.019849220913754625, 0.789436846978699, 0.6135107766465454},
        {-0.009291339744254943, -0.4328980019329044, -0.9013950249076462},
        {-0.769463917170776, -0.3380687171064115, -0.5418808196330908},
        {-0.9985513880836484, -0.05205806143715145, -0.01360454319794869},
    };
    static constexpr double W[7][7] = {
        {0.14399978918360182, 0.09472351872677325, -0.2492742402940041, 0.27712148495885836, -0.1381927751270578, 0.16828288650594117, 0.0005704894753190229},
        {-0.24278402001168958, 0.31320095481284704, 0.27243696516368543, 0.18858873606321686, -0.09077579008822584, 0.14527342346423197, -0.03081888971351041},
        {0.22438381057063342, 0.1746632938151101, -0.27190738796983993, 0.0348108626284531, 0.11609498379861327, -0.2619991304978542, 0.33075803142515386},
        {-0.06661899912823394, 0.1897191879020022, 0.07169723193247461, 0.023534311650291437, 0.45413593191625484, 0.04370649327086241, -0.008485403363582394},
        {-0.027363165703172442, -0.17124731896643947, 0.03589403601156061, 0.2492874138715768, 0.12863948329718589, -0.10565825986236098, -0.32360233257322274},
        {-0.14956082166811843, -0.43470150948950126, 0.15722477307704605, 0.15869483252616154, -0.10050935107517296, 0.09394755889119563, 0.021114722323820508},
        {0.17925353335234595, 0.13285524554247966, 0.38231904760522045, 0.05184081872006227, 0.0004532350146349759, 0.026310857718730526, 0.0005308443858965769},
    };
};
template <> struct RotTab<4> {   // condition number 4.82
    static constexpr double P[9][3] = {
        {-0.36016998959245106, 0.30939461818300795, 0.8800866712070831},
        {-0.8897008156869596, 0.32287297362608325, -0.32277778961355025},
        {-0.7344797900070763, -0.6710231728949664, 0.10132788120321679},
        {0.4825442375302787, 0.28610002585335115, 0.8278271764281684},
        {0.9807283822751025, 0.1641266807981899, -0.10599185275401861},
        {-0.9370007254530625, 0.3135906484128676, 0.1539173340739504},
        {0.05634627101498178, 0.5835788434555645, 0.8100992724436752},
        {-0.669772315128042, 0.6381913254846326, 0.3796272882238453},
        {-0.18226136436742846, -0.4031103401812814, 0.8968181804010527},
    };
    static constexpr double W[9][9] = {
        {-0.2590790399260177, -0.016484798757283547, 0.015258600874928422, -0.050435593673626176, 0.024908770950198566, -0.38559831656570004, -0.05242014479603834, -0.11718698167656927, 0.147667710479993},
        {-0.11039891646548845, 0.06725228112117673, -0.528585215221164, 0.10938781370825693, 0.2566728120531586, 0.11185844509674327, 0.008856019127954593, 0.22371996540427094, 0.06221553050758352},
        {0.05683921965419692, 0.038702096745121393, 0.08166259764266327, -0.07125327336696599, -0.07162604659505857, 0.04417540618763054, -0.4048160083540675, 0.1596050844383943, 0.21734727052926459},
        {-0.06840996636790195, 0.2981009466410674, -0.17335942690731262, -0.275907588751871, 0.16710952001000928, -0.2442563478703507, -0.26046412413089287, 0.10743724678898815, 0.14928778672153112},
        {0.019334962885690376, -0.12172425092717219, -0.4230691256555837, -0.1138673005871548, 0.29962410806532264, -0.00909026930935596, 0.10273707568924406, 0.0482716364723652, 0.24637706956818872},
        {0.1282689713758085, 0.06999346951496023, 0.2087287541642103, 0.2601990464037469, 0.005155266706433893, -0.09884050230694419, -0.06283391767423713, -0.10657786114912672, 0.1546774004875726},
        {-0.011357452016197318, 0.05133084791261267, 0.11534620098054227, -0.06276986255745895, -0.3855219857115208, -0.1010544226769255, 0.2008920742505115, 0.061790054777954045, 0.005810605772854758},
        {-0.00786230344472039, -0.15615507636436876, -0.5549053233638733, 0.10499201066008175, -0.06499047279143108, -0.05304111010859883, 0.2678615250668888, -0.14478165760669875, -0.05799436940759614},
        {-0.2483296167237354, 0.2501896890677825, 0.13883389518160177, -0.292728155637654, -0.11630613939328316, -0.04654233709966222, -0.1976920941309918, -0.09706234376472554, 0.25519407926066756},
    };
};

__device__ __forceinline__ bool rot_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }   // false for NaN

// the 2L+1 harmonics of degree L at the unit vector (x, yy, z): sh.h's closed forms ('component' normalisation, polar
// axis y) in fp64
template <int L>
__device__ __forceinline__ void rot_sh(double x, double yy, double z, double* __restrict__ y) {
    const double x2 = x * x, y2 = yy * yy, z2 = z * z;
    if constexpr (L == 1) {
        const double s3 = 1.7320508075688772;
        y[0] = s3 * x, y[1] = s3 * yy, y[2] = s3 * z;
    }
    if constexpr (L == 2) {
        const double s15 = 3.872983346207417, s5 = 2.23606797749979;
        y[0] = s15 * x * z;
        y[1] = s15 * x * yy;
        y[2] = s5 * (y2 - 0.5 * (x2 + z2));
        y[3] = s15 * yy * z;
        y[4] = (0.5 * s15) * (z2 - x2);
    }
    if constexpr (L == 3) {
        const double s7 = 2.6457513110645907;
        const double c0 = s7 * 0.7905694150420949;   // sqrt(5/8)
        const double c1 = s7 * 3.872983346207417;    // sqrt(15)
        const double c2 = s7 * 0.6123724356957945;   // sqrt(3/8)
        y[0] = c0 * x * (3.0 * z2 - x2);
        y[1] = c1 * x * yy * z;
        y[2] = c2 * x * (4.0 * y2 - x2 - z2);
        y[3] = (0.5 * s7) * yy * (2.0 * y2 - 3.0 * x2 - 3.0 * z2);
        y[4] = c2 * z * (4.0 * y2 - x2 - z2);
        y[5] = (0.5 * c1) * yy * (z2 - x2);
        y[6] = c0 * z * (z2 - 3.0 * x2);
    }
    if constexpr (L == 4) {
        // standard real SH table evaluated at (xs, ys, zs) = (z, x, y), times 3 = sqrt(9)
        const double xs = z, ys = x, zs = yy, xs2 = z2, ys2 = x2, zs2 = y2;
        const double a0 = 3.0 * 2.958039891549808;     // sqrt(35)/2
        const double a1 = 3.0 * 2.0916500663351889;    // sqrt(35/8)
        const double a2 = 3.0 * 1.118033988749895;     // sqrt(5)/2
        const double a3 = 3.0 * 0.7905694150420949;    // sqrt(5/8)
        const double a6 = 3.0 * 0.5590169943749475;    // sqrt(5)/4
        const double a8 = 3.0 * 0.739509972887452;     // sqrt(35)/8
        y[0] = a0 * xs * ys * (xs2 - ys2);
        y[1] = a1 * ys * zs * (3.0 * xs2 - ys2);
        y[2] = a2 * xs * ys * (7.0 * zs2 - 1.0);
        y[3] = a3 * ys * zs * (7.0 * zs2 - 3.0);
        y[4] = (3.0 / 8.0) * (35.0 * zs2 * zs2 - 30.0 * zs2 + 3.0);
        y[5] = a3 * xs * zs * (7.0 * zs2 - 3.0);
        y[6] = a6 * (xs2 - ys2) * (7.0 * zs2 - 1.0);
        y[7] = a1 * xs * zs * (xs2 - 3.0 * ys2);
        y[8] = a8 * (xs2 * xs2 - 6.0 * xs2 * ys2 + ys2 * ys2);
    }
}

// D^L of the proper matrix M (rows M[i][.]) into out[(2L+1)^2], row-major; NaN where `bad`
template <int L>
__device__ __forceinline__ void rot_wigner_block(const double (&M)[3][3], bool bad, double* __restrict__ out) {
    constexpr int N = 2 * L + 1;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    if constexpr (L == 0) {
        out[0] = bad ? nan : 1.0;
    } else {
        double acc[N][N];
#pragma unroll
        for (int i = 0; i < N; ++i) {
#pragma unroll
            for (int j = 0; j < N; ++j) acc[i][j] = 0.0;
        }
#pragma unroll
        for (int k = 0; k < N; ++k) {
            const double px = RotTab<L>::P[k][0], py = RotTab<L>::P[k][1], pz = RotTab<L>::P[k][2];
            const double vx = (M[0][0] * px + M[0][1] * py) + M[0][2] * pz;
            const double vy = (M[1][0] * px + M[1][1] * py) + M[1][2] * pz;
            const double vz = (M[2][0] * px + M[2][1] * py) + M[2][2] * pz;
            // the harmonics normalise their argument: a matrix within orth_tol of orthogonal gives its nearest D to first order
            const double inv = 1.0 / sqrt((vx * vx + vy * vy) + vz * vz);
            double y[N];
            rot_sh<L>(vx * inv, vy * inv, vz * inv, y);
#pragma unroll
            for (int i = 0; i < N; ++i) {
#pragma unroll
                for (int j = 0; j < N; ++j) acc[i][j] = fma(y[i], RotTab<L>::W[k][j], acc[i][j]);
            }
        }
#pragma unroll
        for (int i = 0; i < N; ++i) {
#pragma unroll
            for (int j = 0; j < N; ++j) out[i * N + j] = bad ? nan : acc[i][j];
        }
    }
}

// block b: rotations (b / (lmax+1)) * ROT_THREADS .., degree b % (lmax+1) (uniform per block); the degree-0 block writes the flags
__global__ void __launch_bounds__(ROT_THREADS) rot_wigner_kernel(const double* __restrict__ R, int64_t G, int lmax, double orth_tol,
                                                                 double* __restrict__ D, int32_t* __restrict__ flags) {
    const int nl = lmax + 1;
    const int l = (int)(blockIdx.x % (unsigned)nl);
    const int64_t g = (int64_t)(blockIdx.x / (unsigned)nl) * ROT_THREADS + threadIdx.x;
    if (g >= G) return;

    double M[3][3];
    bool finite = true;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            M[i][j] = R[g * 9 + i * 3 + j];
            finite = finite && rot_finite(M[i][j]);
        }
    }
    double worst = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = i; j < 3; ++j) {
            const double d = (M[0][i] * M[0][j] + M[1][i] * M[1][j]) + M[2][i] * M[2][j] - (i == j ? 1.0 : 0.0);
            worst = fmax(worst, fabs(d));
        }
    }
    const bool skew = finite && !(worst <= orth_tol);
    const double det = M[0][0] * (M[1][1] * M[2][2] - M[1][2] * M[2][1]) - M[0][1] * (M[1][0] * M[2][2] - M[1][2] * M[2][0]) +
                       M[0][2] * (M[1][0] * M[2][1] - M[1][1] * M[2][0]);
    const bool improper = finite && det < 0.0;
    const bool bad = !finite || skew;
    if (improper) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int j = 0; j < 3; ++j) M[i][j] = -M[i][j];
        }
    }
    double* out = D + g * ROT_STRIDE;
    switch (l) {
        case 0:
            rot_wigner_block<0>(M, bad, out + rot_block_offset(0));
            flags[g] = (finite ? 0 : 1) | (skew ? 2 : 0) | (improper ? 4 : 0);
            break;
        case 1: rot_wigner_block<1>(M, bad, out + rot_block_offset(1)); break;
        case 2: rot_wigner_block<2>(M, bad, out + rot_block_offset(2)); break;
        case 3: rot_wigner_block<3>(M, bad, out + rot_block_offset(3)); break;
        default: rot_wigner_block<4>(M, bad, out + rot_block_offset(4)); break;
    }
}

// the layout rows, passed by value; read with compile-time indices only
struct RotLayout {
    int off[ROT_MAX_K], mul[ROT_MAX_K], l[ROT_MAX_K], par[ROT_MAX_K];
};

// irrep copy c of the layout (0 <= c < sum of mul): its first column, degree and parity
__device__ __forceinline__ void rot_find_copy(const RotLayout& lay, int K, int c, int& off, int& l, int& par) {
    off = 0, l = 0, par = 1;
    int first = 0;
#pragma unroll
    for (int k = 0; k < ROT_MAX_K; ++k) {
        const int mul = k < K ? lay.mul[k] : 0;
        const bool hit = c >= first && c < first + mul;
        off = hit ? lay.off[k] + (c - first) * (2 * lay.l[k] + 1) : off;
        l = hit ? lay.l[k] : l;
        par = hit ? lay.par[k] : par;
        first += mul;
    }
}

// y = s D x or s D^T x for one block of degree L, Dl [(2L+1)^2] row-major
template <int L>
__device__ __forceinline__ void rot_matvec(const double* __restrict__ Dl, const double* x, double s, int transpose, double* y) {
    constexpr int N = 2 * L + 1;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        double acc = 0.0;
#pragma unroll
        for (int j = 0; j < N; ++j) acc = fma(transpose ? Dl[j * N + i] : Dl[i * N + j], x[j], acc);
        y[i] = s * acc;
    }
}

template <typename T, int L>
__device__ __forceinline__ void rot_rotate_block(const T* x, T* out, const double* __restrict__ Dl, double s, int transpose,
                                                 bool bad) {
    constexpr int N = 2 * L + 1;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    double xin[N], y[N];
#pragma unroll
    for (int j = 0; j < N; ++j) xin[j] = (double)x[j];
    if (!bad) rot_matvec<L>(Dl, xin, s, transpose, y);
#pragma unroll
    for (int i = 0; i < N; ++i) out[i] = (T)(bad ? nan : y[i]);
}

// block b: rows (b / C) * ROT_THREADS .., irrep copy b % C (uniform per block: one degree, no divergence).  The copies of a
// row sit in neighbouring blocks, so the row's cache lines are shared in L2.  x and out may be the same buffer.
template <typename T>
__global__ void __launch_bounds__(ROT_THREADS) rot_rotate_kernel(const T* x, int64_t n, int64_t dim, RotLayout lay, int K, int C,
                                                                 const double* __restrict__ D, const int32_t* __restrict__ flags,
                                                                 const int32_t* __restrict__ index, int64_t G, int transpose,
                                                                 T* out) {
    const int c = (int)(blockIdx.x % (unsigned)C);
    const int64_t r = (int64_t)(blockIdx.x / (unsigned)C) * ROT_THREADS + threadIdx.x;
    if (r >= n) return;
    int off, l, par;
    rot_find_copy(lay, K, c, off, l, par);
    const int64_t g = index ? (int64_t)index[r] : (G == 1 ? 0 : r);
    const bool bad = g < 0 || g >= G;                      // a row that points at no rotation comes back NaN
    const int64_t gs = bad ? 0 : g;
    const double s = (par < 0 && (flags[gs] & 4)) ? -1.0 : 1.0;
    const double* Dl = D + gs * ROT_STRIDE + rot_block_offset(l);
    const T* xr = x + r * dim + off;
    T* outr = out + r * dim + off;
    switch (l) {
        case 0: rot_rotate_block<T, 0>(xr, outr, Dl, s, transpose, bad); break;
        case 1: rot_rotate_block<T, 1>(xr, outr, Dl, s, transpose, bad); break;
        case 2: rot_rotate_block<T, 2>(xr, outr, Dl, s, transpose, bad); break;
        case 3: rot_rotate_block<T, 3>(xr, outr, Dl, s, transpose, bad); break;
        default: rot_rotate_block<T, 4>(xr, outr, Dl, s, transpose, bad); break;
    }
}

template <typename T, int L>
__device__ __forceinline__ void rot_average_block(const T* x, T* out, const double* __restrict__ D, const int32_t* __restrict__ flags,
                                                  int64_t G, int par, int64_t lo, int64_t hi, const int32_t* __restrict__ op_idx,
                                                  const double* __restrict__ weights, int transpose) {
    constexpr int N = 2 * L + 1;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    double xin[N], acc[N], y[N];
#pragma unroll
    for (int j = 0; j < N; ++j) xin[j] = (double)x[j], acc[j] = 0.0;
    if (hi <= lo) {                                        // the trivial group
#pragma unroll
        for (int i = 0; i < N; ++i) out[i] = x[i];
        return;
    }
    bool bad = false;
    double wsum = 0.0;
    for (int64_t j = lo; j < hi; ++j) {                    // in list order
        const int64_t g = op_idx[j];
        const double w = weights ? weights[j] : 1.0;
        if (g < 0 || g >= G) {                             // points at no rotation: nothing is read, the row comes back NaN
            bad = true;
            continue;
        }
        const int32_t f = flags[g];
        bad = bad || (f & 3) != 0 || !rot_finite(w);
        const double s = (par < 0 && (f & 4)) ? -1.0 : 1.0;
        rot_matvec<L>(D + g * ROT_STRIDE + rot_block_offset(L), xin, s, transpose, y);
#pragma unroll
        for (int i = 0; i < N; ++i) acc[i] = fma(w, y[i], acc[i]);
        wsum += w;
    }
    bad = bad || !(wsum > 0.0);
#pragma unroll
    for (int i = 0; i < N; ++i) out[i] = (T)(bad ? nan : acc[i] / wsum);
}

template <typename T>
__global__ void __launch_bounds__(ROT_THREADS) rot_average_kernel(const T* x, int64_t n, int64_t dim, RotLayout lay, int K, int C,
                                                                  const double* __restrict__ D, const int32_t* __restrict__ flags,
                                                                  int64_t G, const int64_t* __restrict__ op_ptr,
                                                                  const int32_t* __restrict__ op_idx,
                                                                  const double* __restrict__ weights, int transpose, T* out) {
    const int c = (int)(blockIdx.x % (unsigned)C);
    const int64_t r = (int64_t)(blockIdx.x / (unsigned)C) * ROT_THREADS + threadIdx.x;
    if (r >= n) return;
    int off, l, par;
    rot_find_copy(lay, K, c, off, l, par);
    const int64_t lo = op_ptr[r], hi = op_ptr[r + 1];
    const T* xr = x + r * dim + off;
    T* outr = out + r * dim + off;
    switch (l) {
        case 0: rot_average_block<T, 0>(xr, outr, D, flags, G, par, lo, hi, op_idx, weights, transpose); break;
        case 1: rot_average_block<T, 1>(xr, outr, D, flags, G, par, lo, hi, op_idx, weights, transpose); break;
        case 2: rot_average_block<T, 2>(xr, outr, D, flags, G, par, lo, hi, op_idx, weights, transpose); break;
        case 3: rot_average_block<T, 3>(xr, outr, D, flags, G, par, lo, hi, op_idx, weights, transpose); break;
        default: rot_average_block<T, 4>(xr, outr, D, flags, G, par, lo, hi, op_idx, weights, transpose); break;
    }
}

// out[k] = (1 / n) sum_g s D(R_{b,g}) x[src[g,k]] for one block of degree L of atom row k of crystal b, g = 0 .. n-1 in order
template <typename T, int L>
__device__ __forceinline__ void rot_average_atoms_block(const T* x, int64_t dim, int off, T* out, const double* __restrict__ D,
                                                        const int32_t* __restrict__ flags, int par, int64_t n_rows, int64_t k,
                                                        int32_t b, int64_t n_ops, int64_t G_cap,
                                                        const int32_t* __restrict__ row_struct, const int32_t* __restrict__ src) {
    constexpr int N = 2 * L + 1;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    double xin[N], acc[N], y[N];
#pragma unroll
    for (int i = 0; i < N; ++i) acc[i] = 0.0;
    bool bad = n_ops < 1 || n_ops > G_cap;
    const int64_t G = bad ? 0 : n_ops;
    for (int64_t g = 0; g < G; ++g) {
        const int64_t s = src[g * n_rows + k];
        if (s < 0 || s >= n_rows || row_struct[s] != b) {   // no source, or one of another crystal: nothing is read
            bad = true;
            continue;
        }
#pragma unroll
        for (int j = 0; j < N; ++j) xin[j] = (double)x[s * dim + off + j];
        if (D) {
            const int64_t r = (int64_t)b * G_cap + g;
            const int32_t f = flags[r];
            bad = bad || (f & 3) != 0;
            rot_matvec<L>(D + r * ROT_STRIDE + rot_block_offset(L), xin, (par < 0 && (f & 4)) ? -1.0 : 1.0, 0, y);
        } else {
#pragma unroll
            for (int i = 0; i < N; ++i) y[i] = xin[i];
        }
#pragma unroll
        for (int i = 0; i < N; ++i) acc[i] += y[i];
    }
    const double count = (double)n_ops;
#pragma unroll
    for (int i = 0; i < N; ++i) out[i] = (T)(bad ? nan : acc[i] / count);
}

// the grid of rot_rotate_kernel: rows (b / C) * ROT_THREADS .., irrep copy b % C.  out must not be x (rows read their neighbours').
template <typename T>
__global__ void __launch_bounds__(ROT_THREADS) rot_average_atoms_kernel(const T* __restrict__ x, int64_t n, int64_t dim, RotLayout lay,
                                                                        int K, int C, const double* __restrict__ D,
                                                                        const int32_t* __restrict__ flags, int64_t B, int64_t G_cap,
                                                                        const int32_t* __restrict__ n_ops,
                                                                        const int32_t* __restrict__ row_struct,
                                                                        const int32_t* __restrict__ src, T* __restrict__ out) {
    const int c = (int)(blockIdx.x % (unsigned)C);
    const int64_t r = (int64_t)(blockIdx.x / (unsigned)C) * ROT_THREADS + threadIdx.x;
    if (r >= n) return;
    int off, l, par;
    rot_find_copy(lay, K, c, off, l, par);
    const int32_t b = row_struct[r];
    const bool inside = b >= 0 && b < B;                   // a row of no crystal comes back NaN
    const int64_t ops = inside ? (int64_t)n_ops[b] : 0;
    T* outr = out + r * dim + off;
    switch (l) {
        case 0: rot_average_atoms_block<T, 0>(x, dim, off, outr, D, flags, par, n, r, b, ops, G_cap, row_struct, src); break;
        case 1: rot_average_atoms_block<T, 1>(x, dim, off, outr, D, flags, par, n, r, b, ops, G_cap, row_struct, src); break;
        case 2: rot_average_atoms_block<T, 2>(x, dim, off, outr, D, flags, par, n, r, b, ops, G_cap, row_struct, src); break;
        case 3: rot_average_atoms_block<T, 3>(x, dim, off, outr, D, flags, par, n, r, b, ops, G_cap, row_struct, src); break;
        default: rot_average_atoms_block<T, 4>(x, dim, off, outr, D, flags, par, n, r, b, ops, G_cap, row_struct, src); break;
    }
}

// one row per thread, columns in order; reads out as stored (rounded once for fp32 rows)
template <typename T>
__global__ void __launch_bounds__(ROT_THREADS) rot_deviation_kernel(const T* __restrict__ x, const T* __restrict__ out, int64_t n,
                                                                    int64_t dim, double* __restrict__ deviation) {
    const int64_t r = (int64_t)blockIdx.x * ROT_THREADS + threadIdx.x;
    if (r >= n) return;
    double num = 0.0, den = 0.0;
    for (int64_t c = 0; c < dim; ++c) {
        const double a = (double)x[r * dim + c], d = a - (double)out[r * dim + c];
        num = fma(d, d, num);
        den = fma(a, a, den);
    }
    // a NaN row stays NaN, a zero row (x = out = 0) is 0
    deviation[r] = (num == num && den == 0.0) ? 0.0 : sqrt(num) / sqrt(den);
}

}  // namespace

// the layout rows checked on the host and packed for the kernels; C = the number of irrep copies
static bool rot_layout_ok(const int32_t* layout, int K, int64_t dim, RotLayout& lay, int64_t& C) {
    C = 0;
    for (int k = 0; k < ROT_MAX_K; ++k) lay.off[k] = lay.mul[k] = lay.l[k] = 0, lay.par[k] = 1;
    for (int k = 0; k < K; ++k) {
        const int32_t off = layout[4 * k], mul = layout[4 * k + 1], l = layout[4 * k + 2], par = layout[4 * k + 3];
        if (off < 0 || mul < 0 || l < 0 || l > 4 || (par != 1 && par != -1)) return false;
        if ((int64_t)off + (int64_t)mul * (2 * l + 1) > dim) return false;
        lay.off[k] = off, lay.mul[k] = mul, lay.l[k] = l, lay.par[k] = par;
        C += mul;
    }
    // rows must not share columns: two thread groups would write them, and in place one would read what the other wrote
    for (int a = 0; a < K; ++a) {
        for (int b = a + 1; b < K; ++b) {
            const int64_t a_lo = lay.off[a], a_hi = a_lo + (int64_t)lay.mul[a] * (2 * lay.l[a] + 1);
            const int64_t b_lo = lay.off[b], b_hi = b_lo + (int64_t)lay.mul[b] * (2 * lay.l[b] + 1);
            if (a_lo < a_hi && b_lo < b_hi && a_lo < b_hi && b_lo < a_hi) return false;     // (an empty row overlaps nothing)
        }
    }
    return true;
}

static bool rot_grid_ok(int64_t n, int64_t per_row) { return matten_cdiv(n, ROT_THREADS) * per_row <= (int64_t)0x7fffffff; }

extern "C" int matten_wigner_d(const double* R, int64_t G, int lmax, double orth_tol, double* D, int32_t* flags,
                               matten_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (G < 0 || lmax < 0 || lmax > 4 || !(orth_tol >= 0.0) || !rot_grid_ok(G, lmax + 1)) return MATTEN_EINVAL;
    if (G == 0) return MATTEN_OK;
    if (!R || !D || !flags) return MATTEN_EINVAL;
    const unsigned grid = (unsigned)(matten_cdiv(G, ROT_THREADS) * (lmax + 1));
    rot_wigner_kernel<<<grid, ROT_THREADS, 0, stream>>>(R, G, lmax, orth_tol, D, flags);
    MATTEN_LAUNCH_CHECK();
    return MATTEN_OK;
}

extern "C" int matten_irreps_rotate(const void* x, int is_fp64, int64_t n, int64_t dim, const int32_t* layout, int K,
                                    const double* D, const int32_t* flags, const int32_t* index, int64_t G, int transpose,
                                    void* out, matten_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (n < 0 || dim < 0 || K < 0 || K > ROT_MAX_K || G < 0) return MATTEN_EINVAL;
    if ((is_fp64 != 0 && is_fp64 != 1) || (transpose != 0 && transpose != 1)) return MATTEN_EINVAL;
    if (K > 0 && !layout) return MATTEN_EINVAL;
    RotLayout lay;
    int64_t C;
    if (!rot_layout_ok(layout, K, dim, lay, C)) return MATTEN_EINVAL;
    if (n == 0 || G == 0) return MATTEN_OK;
    if (!x || !D || !flags || !out) return MATTEN_EINVAL;
    if (!index && G != 1 && G != n) return MATTEN_EINVAL;
    if (C == 0) return MATTEN_OK;
    if (!rot_grid_ok(n, C)) return MATTEN_EINVAL;
    const unsigned grid = (unsigned)(matten_cdiv(n, ROT_THREADS) * C);
    if (is_fp64)
        rot_rotate_kernel<double><<<grid, ROT_THREADS, 0, stream>>>((const double*)x, n, dim, lay, K, (int)C, D, flags, index, G,
                                                                    transpose, (double*)out);
    else
        rot_rotate_kernel<float><<<grid, ROT_THREADS, 0, stream>>>((const float*)x, n, dim, lay, K, (int)C, D, flags, index, G,
                                                                   transpose, (float*)out);
    MATTEN_LAUNCH_CHECK();
    return MATTEN_OK;
}

extern "C" int matten_irreps_average(const void* x, int is_fp64, int64_t n, int64_t dim, const int32_t* layout, int K,
                                     const double* D, const int32_t* flags, int64_t G, const int64_t* op_ptr,
                                     const int32_t* op_idx, const double* weights, int transpose, void* out,
                                     double* deviation, matten_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (n < 0 || dim < 0 || K < 0 || K > ROT_MAX_K || G < 0) return MATTEN_EINVAL;
    if ((is_fp64 != 0 && is_fp64 != 1) || (transpose != 0 && transpose != 1)) return MATTEN_EINVAL;
    if (K > 0 && !layout) return MATTEN_EINVAL;
    RotLayout lay;
    int64_t C;
    if (!rot_layout_ok(layout, K, dim, lay, C)) return MATTEN_EINVAL;
    if (n == 0) return MATTEN_OK;
    // (G = 0 is allowed here: every row's list may be empty; op_idx, D and flags are then never read)
    if (!x || !op_ptr || !out || (G > 0 && (!D || !flags || !op_idx))) return MATTEN_EINVAL;
    if (!rot_grid_ok(n, C > 0 ? C : 1)) return MATTEN_EINVAL;
    if (C > 0) {
        const unsigned grid = (unsigned)(matten_cdiv(n, ROT_THREADS) * C);
        if (is_fp64)
            rot_average_kernel<double><<<grid, ROT_THREADS, 0, stream>>>((const double*)x, n, dim, lay, K, (int)C, D, flags, G, op_ptr,
                                                                         op_idx, weights, transpose, (double*)out);
        else
            rot_average_kernel<float><<<grid, ROT_THREADS, 0, stream>>>((const float*)x, n, dim, lay, K, (int)C, D, flags, G, op_ptr,
                                                                        op_idx, weights, transpose, (float*)out);
        MATTEN_LAUNCH_CHECK();
    }
    if (deviation) {
        const unsigned grid = (unsigned)matten_cdiv(n, ROT_THREADS);
        if (is_fp64) rot_deviation_kernel<double><<<grid, ROT_THREADS, 0, stream>>>((const double*)x, (const double*)out, n, dim, deviation);
        else rot_deviation_kernel<float><<<grid, ROT_THREADS, 0, stream>>>((const float*)x, (const float*)out, n, dim, deviation);
        MATTEN_LAUNCH_CHECK();
    }
    return MATTEN_OK;
}

extern "C" int matten_irreps_average_atoms(const void* x, int is_fp64, int64_t n, int64_t dim, const int32_t* layout, int K,
                                           const double* D, const int32_t* flags, int64_t B, int64_t G_cap, const int32_t* n_ops,
                                           const int32_t* row_struct, const int32_t* src, void* out, matten_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (n < 0 || dim < 0 || K < 0 || K > ROT_MAX_K || B < 0 || G_cap < 1) return MATTEN_EINVAL;
    if (is_fp64 != 0 && is_fp64 != 1) return MATTEN_EINVAL;
    if (K > 0 && !layout) return MATTEN_EINVAL;
    RotLayout lay;
    int64_t C;
    if (!rot_layout_ok(layout, K, dim, lay, C)) return MATTEN_EINVAL;
    if (!x || !out || x == out || !n_ops || !row_struct || !src || (D && !flags)) return MATTEN_EINVAL;
    if (n > (int64_t)0x7fffffff || !rot_grid_ok(n, C > 0 ? C : 1)) return MATTEN_EINVAL;   // sources are int32 row numbers
    if (n == 0 || C == 0) return MATTEN_OK;
    const unsigned grid = (unsigned)(matten_cdiv(n, ROT_THREADS) * C);
    if (is_fp64)
        rot_average_atoms_kernel<double><<<grid, ROT_THREADS, 0, stream>>>((const double*)x, n, dim, lay, K, (int)C, D, flags, B, G_cap,
                                                                           n_ops, row_struct, src, (double*)out);
    else
        rot_average_atoms_kernel<float><<<grid, ROT_THREADS, 0, stream>>>((const float*)x, n, dim, lay, K, (int)C, D, flags, B, G_cap,
                                                                          n_ops, row_struct, src, (float*)out);
    MATTEN_LAUNCH_CHECK();
    return MATTEN_OK;
}
