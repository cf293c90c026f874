// Symmetry of a batch of crystals, found on the device (include/matten_hip.h, "Finding a crystal's symmetry").
//   sg_lattice_kernel  : the integer matrices N with N G N^T = G to tolerance (the lattice's point group), one workgroup per
//                        crystal: candidate rows into LDS, the triple loop over them spread over the threads, kept in
//                        enumeration order by a ballot prefix sum
//   sg_search_kernel   : one wave per (crystal, lattice operation): candidate translations from the pivot species, an atom
//                        at a time against all atoms across the lanes, abandoned at the first atom without an image
//   sg_finalize_kernel : one workgroup per crystal: flags, compaction of the accepted operations to lattice order, the
//                        Cartesian matrices (polar factor of (L^-1 N L)^T by sym3.h's Jacobi), -1 fill of absent rows
// The reference has no symmetry search (it reads space groups from pymatgen on the host).  fp64 throughout.  No atomics, no
// allocation, nothing read back; every output word has one writer per launch: two runs are bit-identical and capturable.
#include "common.h"
#include "sym3.h"

namespace {

constexpr int SG_OPS = MATTEN_SYM_MAX_OPS;         // 48
constexpr int SG_MAX_ATOMS = MATTEN_SYM_MAX_ATOMS; // 1024: the fractional coordinates, species and two maps take 32 KB of LDS
constexpr int SG_MAX_M = 4;                        // |n_j| <= 4 per row entry
constexpr int SG_SIDE = 2 * SG_MAX_M + 1;
constexpr int SG_CAND = SG_SIDE * SG_SIDE * SG_SIDE;   // 729 candidate rows at most
constexpr int SG_LAT_THREADS = 256;
constexpr int SG_FIN_THREADS = 256;
constexpr int SG_WAVE = 64;
constexpr int SG_MARK_AMBIGUOUS = 127;             // first entry of a rot_int slot between search and finalize
constexpr double SG_SINGULAR = 1e-12;              // |det L| at or below: singular (predict.pack_structures' threshold)

__device__ __forceinline__ bool sg_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }   // false for NaN

struct SgCell {
    double L[3][3], Li[3][3], G[3][3], amax;
    bool ok;                                       // finite and not singular
};

// L (rows = lattice vectors), its inverse (f = r Li), the metric G = L L^T and the longest vector
__device__ __forceinline__ void sg_cell(const double* __restrict__ cell, SgCell& c) {
    bool finite = true;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            c.L[i][j] = cell[i * 3 + j];
            finite = finite && sg_finite(c.L[i][j]);
        }
    }
    const double (&L)[3][3] = c.L;
    const double c00 = L[1][1] * L[2][2] - L[1][2] * L[2][1], c01 = L[1][2] * L[2][0] - L[1][0] * L[2][2],
                 c02 = L[1][0] * L[2][1] - L[1][1] * L[2][0];
    const double det = (L[0][0] * c00 + L[0][1] * c01) + L[0][2] * c02;
    c.ok = finite && fabs(det) > SG_SINGULAR;
    const double inv = 1.0 / det;
    c.Li[0][0] = c00 * inv, c.Li[1][0] = c01 * inv, c.Li[2][0] = c02 * inv;
    c.Li[0][1] = (L[0][2] * L[2][1] - L[0][1] * L[2][2]) * inv;
    c.Li[1][1] = (L[0][0] * L[2][2] - L[0][2] * L[2][0]) * inv;
    c.Li[2][1] = (L[0][1] * L[2][0] - L[0][0] * L[2][1]) * inv;
    c.Li[0][2] = (L[0][1] * L[1][2] - L[0][2] * L[1][1]) * inv;
    c.Li[1][2] = (L[0][2] * L[1][0] - L[0][0] * L[1][2]) * inv;
    c.Li[2][2] = (L[0][0] * L[1][1] - L[0][1] * L[1][0]) * inv;
    double gmax = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) c.G[i][j] = (L[i][0] * L[j][0] + L[i][1] * L[j][1]) + L[i][2] * L[j][2];
        gmax = fmax(gmax, c.G[i][i]);
    }
    c.amax = sqrt(gmax);
}

// a G b^T for integer rows
__device__ __forceinline__ double sg_form(const double (&G)[3][3], const int (&a)[3], const int (&b)[3]) {
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double gi = ((double)b[0] * G[i][0] + (double)b[1] * G[i][1]) + (double)b[2] * G[i][2];
        s = fma((double)a[i], gi, s);
    }
    return s;
}

// rank of this thread's hit among the hits of the workgroup (4 waves) in thread order, and their number; every thread calls it
__device__ __forceinline__ int sg_block_rank(bool hit, int* wave_cnt, int& total) {
    const unsigned long long mask = __ballot(hit);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    __syncthreads();                               // the previous call's readers are done
    if (lane == 0) wave_cnt[w] = __popcll(mask);
    __syncthreads();
    int before = 0;
    total = 0;
#pragma unroll
    for (int v = 0; v < SG_LAT_THREADS / 64; ++v) {
        const int c = wave_cnt[v];
        before += v < w ? c : 0;
        total += c;
    }
    return before + __popcll(mask & ((1ull << lane) - 1ull));
}

__global__ void __launch_bounds__(SG_LAT_THREADS) sg_lattice_kernel(const double* __restrict__ cell, double symprec,
                                                                    int8_t* __restrict__ N_out, int32_t* __restrict__ n_lat,
                                                                    int32_t* __restrict__ flags) {
    __shared__ int8_t cand[3][SG_CAND][3];
    __shared__ int wave_cnt[SG_LAT_THREADS / 64];
    const int64_t b = blockIdx.x;
    const int t = threadIdx.x;
    SgCell c;
    sg_cell(cell + b * 9, c);
    int m[3] = {0, 0, 0};
    bool range = false;
    if (c.ok) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const double astar = sqrt((c.Li[0][j] * c.Li[0][j] + c.Li[1][j] * c.Li[1][j]) + c.Li[2][j] * c.Li[2][j]);
            const double mj = floor((c.amax + symprec) * astar);
            range = range || !(mj <= (double)SG_MAX_M);
            m[j] = range ? 0 : (int)mj;
        }
    }
    int8_t* out = N_out + b * (SG_OPS * 9);
    for (int e = t; e < SG_OPS * 9; e += SG_LAT_THREADS) out[e] = (e == 0 || e == 4 || e == 8) ? 1 : 0;   // the identity, zeros
    if (!c.ok || range) {                          // (uniform over the workgroup)
        if (t == 0) n_lat[b] = 1, flags[b] = (c.ok ? 0 : MATTEN_SYM_NOT_FINITE) | (range ? MATTEN_SYM_RANGE : 0);
        return;
    }
    const double tol = 2.0 * symprec * c.amax;
    const int s1 = 2 * m[1] + 1, s2 = 2 * m[2] + 1, total = (2 * m[0] + 1) * s1 * s2;   // <= 729
    int ncand[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        int base = 0;
        for (int chunk = 0; chunk < total; chunk += SG_LAT_THREADS) {
            const int e = chunk + t;
            int n[3] = {0, 0, 0};
            bool hit = false;
            if (e < total) {
                n[0] = e / (s1 * s2) - m[0], n[1] = (e / s2) % s1 - m[1], n[2] = e % s2 - m[2];
                hit = fabs(sg_form(c.G, n, n) - c.G[i][i]) <= tol;
            }
            int hits;
            const int r = sg_block_rank(hit, wave_cnt, hits);
            if (hit) cand[i][base + r][0] = (int8_t)n[0], cand[i][base + r][1] = (int8_t)n[1], cand[i][base + r][2] = (int8_t)n[2];
            base += hits;
        }
        ncand[i] = base;
    }
    __syncthreads();
    // rows ascend lexicographically within each list, so the triples (i0, i1, i2) ascend in the nine entries row-major
    const int64_t ncomb = (int64_t)ncand[0] * ncand[1] * ncand[2];
    int count = 1;                                 // the identity is first, whatever its place in the enumeration
    for (int64_t chunk = 0; chunk < ncomb && count <= SG_OPS; chunk += SG_LAT_THREADS) {
        const int64_t e = chunk + t;
        int r[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
        bool hit = false;
        if (e < ncomb) {
            const int i0 = (int)(e / ((int64_t)ncand[1] * ncand[2])), i1 = (int)((e / ncand[2]) % ncand[1]), i2 = (int)(e % ncand[2]);
#pragma unroll
            for (int k = 0; k < 3; ++k) r[0][k] = cand[0][i0][k], r[1][k] = cand[1][i1][k], r[2][k] = cand[2][i2][k];
            hit = fabs(sg_form(c.G, r[0], r[1]) - c.G[0][1]) <= tol && fabs(sg_form(c.G, r[0], r[2]) - c.G[0][2]) <= tol &&
                  fabs(sg_form(c.G, r[1], r[2]) - c.G[1][2]) <= tol;
            const bool identity = r[0][0] == 1 && r[0][1] == 0 && r[0][2] == 0 && r[1][0] == 0 && r[1][1] == 1 && r[1][2] == 0 &&
                                  r[2][0] == 0 && r[2][1] == 0 && r[2][2] == 1;
            hit = hit && !identity;
        }
        int hits;
        const int slot = count + sg_block_rank(hit, wave_cnt, hits);
        if (hit && slot < SG_OPS) {
#pragma unroll
            for (int k = 0; k < 9; ++k) out[slot * 9 + k] = (int8_t)r[k / 3][k % 3];
        }
        count += hits;
    }
    if (count > SG_OPS) {                          // more than a point group holds: symprec is too large for this cell
        __syncthreads();
        for (int e = 9 + t; e < SG_OPS * 9; e += SG_LAT_THREADS) out[e] = 0;
    }
    if (t == 0) n_lat[b] = count > SG_OPS ? 1 : count, flags[b] = count > SG_OPS ? MATTEN_SYM_AMBIGUOUS : 0;
}

// crystals that the search leaves alone: the finalize kernel writes their identity without reading a slot
__device__ __forceinline__ bool sg_skip(int32_t lat_flag, int64_t n, const uint8_t* __restrict__ pbc, int64_t b) {
    const bool open = pbc && !(pbc[b * 3] && pbc[b * 3 + 1] && pbc[b * 3 + 2]);
    return lat_flag != 0 || n < 1 || n > SG_MAX_ATOMS || open;
}

__device__ __forceinline__ double sg_wrap(double v) { return v - rint(v); }

// block (b, g): lattice operation g of crystal b.  One wave.  For every candidate translation t = f_j - f_p N (j over the pivot
// species, ascending) atom i = 0, 1, .. is imaged and tested against all atoms k across the lanes; the first atom without an
// image ends the candidate.  g > 0 stops at its first accepted j (the representative); g = 0 (the identity) goes on and
// lists the pure translations.  The slot rot_int[b,g] tells the finalize kernel the outcome: zeros = not an operation,
// N = accepted, 127.. = accepted but ambiguous.
__global__ void __launch_bounds__(SG_WAVE) sg_search_kernel(const double* __restrict__ pos, const double* __restrict__ cell,
                                                            const int64_t* __restrict__ Z, const int64_t* __restrict__ ptr,
                                                            const uint8_t* __restrict__ pbc, int64_t N_total, double symprec,
                                                            int max_trans, const int8_t* __restrict__ N_in,
                                                            const int32_t* __restrict__ n_lat, const int32_t* __restrict__ lat_flags,
                                                            int8_t* __restrict__ rot_int, double* __restrict__ trans,
                                                            int32_t* __restrict__ src, int32_t* __restrict__ n_trans,
                                                            double* __restrict__ ttrans, int32_t* __restrict__ tsrc) {
    __shared__ double f[3][SG_MAX_ATOMS];
    __shared__ int32_t zs[SG_MAX_ATOMS];
    __shared__ int16_t img[SG_MAX_ATOMS];          // img[i] = k: atom i lands on atom k
    __shared__ int16_t inv[SG_MAX_ATOMS];          // inv[k] = i
    const int64_t b = blockIdx.x / SG_OPS;
    const int g = (int)(blockIdx.x % SG_OPS);
    const int lane = threadIdx.x;
    const int64_t lo = ptr[b], n64 = ptr[b + 1] - lo;
    if (sg_skip(lat_flags[b], n64, pbc, b)) return;
    const int n = (int)n64;
    int8_t* slot = rot_int + (b * SG_OPS + g) * 9;
    if (g >= n_lat[b]) {
        if (lane < 9) slot[lane] = 0;
        return;
    }
    SgCell c;
    sg_cell(cell + b * 9, c);
    for (int k = lane; k < n; k += SG_WAVE) {
        const double x = pos[(lo + k) * 3], y = pos[(lo + k) * 3 + 1], z = pos[(lo + k) * 3 + 2];
#pragma unroll
        for (int d = 0; d < 3; ++d) f[d][k] = (x * c.Li[0][d] + y * c.Li[1][d]) + z * c.Li[2][d];
        zs[k] = (int32_t)Z[lo + k];
    }
    __syncthreads();
    // the pivot: the lowest-indexed atom of the species with the fewest atoms, ties to the smallest Z
    unsigned long long key = ~0ull;
    for (int k = lane; k < n; k += SG_WAVE) {
        const int32_t zk = zs[k];
        int cnt = 0;
        for (int j = 0; j < n; ++j) cnt += zs[j] == zk ? 1 : 0;
        const unsigned long long mine = ((unsigned long long)cnt << 44) | ((unsigned long long)((uint32_t)zk ^ 0x80000000u) << 12) |
                                        (unsigned long long)k;
        key = mine < key ? mine : key;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long other = __shfl_xor(key, off);
        key = other < key ? other : key;
    }
    const int p = (int)(key & 0xfffull);
    const int32_t zp = zs[p];
    double Nd[3][3];
#pragma unroll
    for (int i = 0; i < 9; ++i) Nd[i / 3][i % 3] = (double)N_in[(b * SG_OPS + g) * 9 + i];
    double fpN[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) fpN[d] = (f[0][p] * Nd[0][d] + f[1][p] * Nd[1][d]) + f[2][p] * Nd[2][d];
    const double sp2 = symprec * symprec;

    int n_found = 0;
    bool any_ambiguous = false, accepted_any = false;
    for (int j = 0; j < n; ++j) {                  // (uniform over the wave, like every loop below)
        if (zs[j] != zp) continue;
        const double t0 = f[0][j] - fpN[0], t1 = f[1][j] - fpN[1], t2 = f[2][j] - fpN[2];
        bool accepted = true, multi = false;
        for (int i = 0; i < n; ++i) {
            const double a0 = f[0][i], a1 = f[1][i], a2 = f[2][i];
            const double i0 = ((a0 * Nd[0][0] + a1 * Nd[1][0]) + a2 * Nd[2][0]) + t0;
            const double i1 = ((a0 * Nd[0][1] + a1 * Nd[1][1]) + a2 * Nd[2][1]) + t1;
            const double i2 = ((a0 * Nd[0][2] + a1 * Nd[1][2]) + a2 * Nd[2][2]) + t2;
            const int32_t zi = zs[i];
            int cnt = 0, first = -1;
            for (int k0 = 0; k0 < n; k0 += SG_WAVE) {
                const int k = k0 + lane;
                bool hit = false;
                if (k < n && zs[k] == zi) {
                    const double d0 = sg_wrap(i0 - f[0][k]), d1 = sg_wrap(i1 - f[1][k]), d2 = sg_wrap(i2 - f[2][k]);
                    const double x = (d0 * c.L[0][0] + d1 * c.L[1][0]) + d2 * c.L[2][0];
                    const double y = (d0 * c.L[0][1] + d1 * c.L[1][1]) + d2 * c.L[2][1];
                    const double z = (d0 * c.L[0][2] + d1 * c.L[1][2]) + d2 * c.L[2][2];
                    hit = (x * x + y * y) + z * z <= sp2;
                }
                const unsigned long long mask = __ballot(hit);
                if (mask != 0ull && first < 0) first = k0 + __ffsll((long long)mask) - 1;
                cnt += __popcll(mask);
            }
            if (cnt == 0) {
                accepted = false;
                break;
            }
            multi = multi || cnt > 1;
            if (lane == 0) img[i] = (int16_t)first;
        }
        if (!accepted) continue;
        // the inverse map; two atoms on one k leave an i whose k names another
        __syncthreads();
        for (int k = lane; k < n; k += SG_WAVE) inv[k] = -1;
        __syncthreads();
        for (int i = lane; i < n; i += SG_WAVE) inv[img[i]] = (int16_t)i;
        __syncthreads();
        bool dup = false;
        for (int i = lane; i < n; i += SG_WAVE) dup = dup || inv[img[i]] != i;
        const bool ambiguous = multi || __ballot(dup) != 0ull;
        any_ambiguous = any_ambiguous || ambiguous;
        accepted_any = true;
        if (g != 0 || n_found == 0) {              // the representative of this lattice operation (j = p for the identity)
            for (int k = lane; k < n; k += SG_WAVE) src[(int64_t)g * N_total + lo + k] = (int32_t)(lo + inv[k]);
            if (lane == 0) {
                double* tr = trans + (b * SG_OPS + g) * 3;
                tr[0] = t0, tr[1] = t1, tr[2] = t2;
            }
        }
        if (g != 0) break;
        if (n_found < max_trans) {
            for (int k = lane; k < n; k += SG_WAVE) tsrc[(int64_t)n_found * N_total + lo + k] = (int32_t)(lo + inv[k]);
            if (lane == 0) {
                double* tr = ttrans + (b * (int64_t)max_trans + n_found) * 3;
                tr[0] = t0, tr[1] = t1, tr[2] = t2;
            }
        }
        ++n_found;
        __syncthreads();                           // inv is cleared again for the next translation
    }
    if (lane < 9) {
        const int8_t v = N_in[(b * SG_OPS + g) * 9 + lane];
        slot[lane] = !accepted_any ? (int8_t)0 : any_ambiguous ? (int8_t)SG_MARK_AMBIGUOUS : v;
    }
    if (g == 0 && lane == 0) n_trans[b] = n_found;
}

// the nearest orthogonal matrix of M = (Li N L)^T: M (M^T M)^-1/2
__device__ __forceinline__ void sg_polar(const SgCell& c, const int (&N)[9], double* __restrict__ out) {
    double NL[3][3], M[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) NL[i][j] = ((double)N[i * 3] * c.L[0][j] + (double)N[i * 3 + 1] * c.L[1][j]) + (double)N[i * 3 + 2] * c.L[2][j];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) M[j][i] = (c.Li[i][0] * NL[0][j] + c.Li[i][1] * NL[1][j]) + c.Li[i][2] * NL[2][j];
    }
    double S[3][3], lam[3], U[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) S[i][j] = (M[0][i] * M[0][j] + M[1][i] * M[1][j]) + M[2][i] * M[2][j];
    }
    sym3_eig<true>(S, lam, U);
    double W[3][3];                                // (M^T M)^-1/2 = U diag(lam^-1/2) U^T
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j)
            W[i][j] = (U[i][0] * U[j][0] / sqrt(lam[0]) + U[i][1] * U[j][1] / sqrt(lam[1])) + U[i][2] * U[j][2] / sqrt(lam[2]);
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) out[i * 3 + j] = (M[i][0] * W[0][j] + M[i][1] * W[1][j]) + M[i][2] * W[2][j];
    }
}

__global__ void __launch_bounds__(SG_FIN_THREADS) sg_finalize_kernel(const double* __restrict__ pos, const double* __restrict__ cell,
                                                                     const int64_t* __restrict__ ptr, const uint8_t* __restrict__ pbc,
                                                                     int64_t N_total, int max_trans,
                                                                     const int32_t* __restrict__ lat_flags, double* __restrict__ rot,
                                                                     int8_t* __restrict__ rot_int, double* __restrict__ trans,
                                                                     int32_t* __restrict__ n_rot, int32_t* __restrict__ src,
                                                                     int32_t* __restrict__ n_trans, double* __restrict__ ttrans,
                                                                     int32_t* __restrict__ tsrc, int32_t* __restrict__ flags) {
    __shared__ int rank_s[SG_OPS];                 // the slot an accepted operation moves to, -1 otherwise
    __shared__ int nrot_s;
    const int64_t b = blockIdx.x;
    const int t = threadIdx.x;
    const int64_t lo = ptr[b], n = ptr[b + 1] - lo;
    const int32_t lat_flag = lat_flags[b];
    int fl = lat_flag;
    if (n < 1) fl |= MATTEN_SYM_NOT_FINITE;
    if (n > SG_MAX_ATOMS) fl |= MATTEN_SYM_TOO_LARGE;
    if (pbc && !(pbc[b * 3] && pbc[b * 3 + 1] && pbc[b * 3 + 2])) fl |= MATTEN_SYM_NOT_PERIODIC;
    bool bad = false;
    for (int64_t e = t; e < n * 3; e += SG_FIN_THREADS) bad = bad || !sg_finite(pos[lo * 3 + e]);
    if (__syncthreads_or(bad ? 1 : 0)) fl |= MATTEN_SYM_NOT_FINITE;
    const bool searched = !sg_skip(lat_flag, n, pbc, b);   // (uniform)

    int N[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    double tr[3] = {0.0, 0.0, 0.0};
    bool accepted = false, marked = false;
    if (searched && t < SG_OPS) {
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            N[k] = rot_int[(b * SG_OPS + t) * 9 + k];
            accepted = accepted || N[k] != 0;
        }
        marked = N[0] == SG_MARK_AMBIGUOUS;
        if (accepted) {
#pragma unroll
            for (int d = 0; d < 3; ++d) tr[d] = trans[(b * SG_OPS + t) * 3 + d];
        }
    }
    if (__syncthreads_or(marked ? 1 : 0)) fl |= MATTEN_SYM_AMBIGUOUS;
    // (a crystal with a non-finite coordinate fails its own identity; bit 0 is already set)
    if (t < SG_OPS) rank_s[t] = accepted ? 1 : 0;
    __syncthreads();
    if (t == 0) {
        int r = 0;
        for (int g = 0; g < SG_OPS; ++g) {
            const int a = rank_s[g];
            rank_s[g] = a ? r : -1;
            r += a;
        }
        nrot_s = r;
    }
    __syncthreads();
    const int identity_only = MATTEN_SYM_NOT_FINITE | MATTEN_SYM_RANGE | MATTEN_SYM_TOO_LARGE | MATTEN_SYM_AMBIGUOUS | MATTEN_SYM_NOT_PERIODIC;
    if ((fl & identity_only) != 0 || nrot_s < 1 || rank_s[0] != 0) {
        if (nrot_s < 1 || rank_s[0] != 0) fl |= (fl & identity_only) ? 0 : MATTEN_SYM_NOT_FINITE;
        if (t < SG_OPS) {
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                const bool one = t == 0 && (k == 0 || k == 4 || k == 8);
                rot_int[(b * SG_OPS + t) * 9 + k] = one ? 1 : 0;
                rot[(b * SG_OPS + t) * 9 + k] = one ? 1.0 : 0.0;
            }
#pragma unroll
            for (int d = 0; d < 3; ++d) trans[(b * SG_OPS + t) * 3 + d] = 0.0;
        }
        for (int64_t e = t; e < (int64_t)max_trans * 3; e += SG_FIN_THREADS) ttrans[b * (int64_t)max_trans * 3 + e] = 0.0;
        for (int64_t k = t; k < n; k += SG_FIN_THREADS) {
            for (int g = 0; g < SG_OPS; ++g) src[(int64_t)g * N_total + lo + k] = g == 0 ? (int32_t)(lo + k) : -1;
            for (int tau = 0; tau < max_trans; ++tau) tsrc[(int64_t)tau * N_total + lo + k] = tau == 0 ? (int32_t)(lo + k) : -1;
        }
        if (t == 0) n_rot[b] = 1, n_trans[b] = 1, flags[b] = fl;
        return;
    }
    const int nrot = nrot_s;
    // every accepted slot was read above; now each moves down to its rank and the rest are cleared
    if (t < SG_OPS) {
        const int r = rank_s[t];
        if (r >= 0) {
            SgCell c;
            sg_cell(cell + b * 9, c);
            sg_polar(c, N, rot + (b * SG_OPS + r) * 9);
#pragma unroll
            for (int k = 0; k < 9; ++k) rot_int[(b * SG_OPS + r) * 9 + k] = (int8_t)N[k];
#pragma unroll
            for (int d = 0; d < 3; ++d) trans[(b * SG_OPS + r) * 3 + d] = sg_wrap(tr[d]);
        }
        if (t >= nrot) {
#pragma unroll
            for (int k = 0; k < 9; ++k) rot_int[(b * SG_OPS + t) * 9 + k] = 0, rot[(b * SG_OPS + t) * 9 + k] = 0.0;
#pragma unroll
            for (int d = 0; d < 3; ++d) trans[(b * SG_OPS + t) * 3 + d] = 0.0;
        }
    }
    const int nt = n_trans[b];
    const int kept = nt < max_trans ? nt : max_trans;
    for (int64_t e = t; e < (int64_t)max_trans * 3; e += SG_FIN_THREADS) {
        double* w = ttrans + b * (int64_t)max_trans * 3 + e;
        *w = e < (int64_t)kept * 3 ? sg_wrap(*w) : 0.0;
    }
    for (int64_t k = t; k < n; k += SG_FIN_THREADS) {     // a column per thread: rank <= slot, ascending, so nothing unread is lost
        for (int g = 0; g < SG_OPS; ++g) {
            const int r = rank_s[g];
            if (r >= 0 && r != g) src[(int64_t)r * N_total + lo + k] = src[(int64_t)g * N_total + lo + k];
        }
        for (int g = nrot; g < SG_OPS; ++g) src[(int64_t)g * N_total + lo + k] = -1;
        for (int tau = kept; tau < max_trans; ++tau) tsrc[(int64_t)tau * N_total + lo + k] = -1;
    }
    if (t == 0) n_rot[b] = nrot, flags[b] = fl | (nt > max_trans ? MATTEN_SYM_TRUNC : 0);
}

}  // namespace

static bool sg_symprec_ok(double symprec) { return symprec > 0.0 && symprec <= 1.7976931348623157e308; }

extern "C" int matten_lattice_group(const double* cell, int64_t B, double symprec, int8_t* N_out, int32_t* n_lat, int32_t* flags,
                                    matten_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (B < 0 || B > (int64_t)0x7fffffff || !sg_symprec_ok(symprec)) return MATTEN_EINVAL;
    if (!cell || !N_out || !n_lat || !flags) return MATTEN_EINVAL;
    if (B == 0) return MATTEN_OK;
    sg_lattice_kernel<<<(unsigned)B, SG_LAT_THREADS, 0, stream>>>(cell, symprec, N_out, n_lat, flags);
    MATTEN_LAUNCH_CHECK();
    return MATTEN_OK;
}

extern "C" int matten_crystal_symmetry(const double* pos, const double* cell, const int64_t* Z, const int64_t* ptr,
                                       const uint8_t* pbc, int64_t B, int64_t N_total, double symprec, int max_trans,
                                       const int8_t* N_in, const int32_t* n_lat, const int32_t* lat_flags, double* rot,
                                       int8_t* rot_int, double* trans, int32_t* n_rot, int32_t* src, int32_t* n_trans,
                                       double* ttrans, int32_t* tsrc, int32_t* flags, matten_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (B < 0 || N_total < 0 || max_trans < 1 || !sg_symprec_ok(symprec)) return MATTEN_EINVAL;
    // atom indices are int32, and so are the grids (B * 48 blocks)
    if (N_total > (int64_t)0x7fffffff || B * SG_OPS > (int64_t)0x7fffffff) return MATTEN_EINVAL;
    if (!pos || !cell || !Z || !ptr || !N_in || !n_lat || !lat_flags) return MATTEN_EINVAL;
    if (!rot || !rot_int || !trans || !n_rot || !src || !n_trans || !ttrans || !tsrc || !flags) return MATTEN_EINVAL;
    if (B == 0) return MATTEN_OK;
    sg_search_kernel<<<(unsigned)(B * SG_OPS), SG_WAVE, 0, stream>>>(pos, cell, Z, ptr, pbc, N_total, symprec, max_trans, N_in, n_lat,
                                                                      lat_flags, rot_int, trans, src, n_trans, ttrans, tsrc);
    MATTEN_LAUNCH_CHECK();
    sg_finalize_kernel<<<(unsigned)B, SG_FIN_THREADS, 0, stream>>>(pos, cell, ptr, pbc, N_total, max_trans, lat_flags, rot, rot_int,
                                                                   trans, n_rot, src, n_trans, ttrans, tsrc, flags);
    MATTEN_LAUNCH_CHECK();
    return MATTEN_OK;
}
