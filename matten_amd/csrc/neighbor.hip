// Periodic neighbour list on the GPU, canonical order.
// Contract of the reference's graph builder (data/data.py:285-413, which calls ASE): every ordered triple
// (i, j, S) with | r_j + S.cell - r_i | < r_cut (strict, fp64), minus the true self edge (i == j, S == 0);
// edge_index[0] = i (centre), edge_index[1] = j, edge_cell_shift = S.  Edges are emitted in the
// lexicographic order (i, j, Sx, Sy, Sz) so the result is deterministic and identical to the host builder.
//
// matten_graph_prep (one wave per crystal) turns the four arrays that cross PCIe into what the search needs: inverse
// cell in closed form, fractional coordinates, the per-axis bound r_cut |inv[:, k]| and the fp32 / index copies the
// model takes.  One thread per ordered atom PAIR (i, j) of a crystal then walks only the image shifts that can hold a
// neighbour: d . inv[:, k] = S_k + (f_j - f_i)_k and |d . inv[:, k]| <= |d| |inv[:, k]| < r_cut |inv[:, k]|, so
// S_k lies in [-bound_k - df_k, bound_k - df_k] (widened by 1e-6 relative: the bound only prunes, the exact test
// decides) -- ~2 values per axis instead of the 2 reach + 1 of a per-crystal box (5^3 = 125 images per pair for an
// fcc-64 cell, 8 now).  The shifts are walked in lexicographic order twice: a counting pass, then (after an exclusive
// scan of the per-pair counts by the caller) a fill pass that writes the pair's edges contiguously.  Pairs are
// numbered crystal by crystal, i-major, so the scan order IS the canonical edge order.
// The destination-sorted CSR the conv layers walk (destination = edge_index[1] = j, stable in the edge id: what
// matten_csr_build derives from the finished list in seven launches) falls out of the same two passes: the counting
// pass also stores each pair's count at its TRANSPOSED (j-major) pair number, the caller scans those too, and the fill
// pass drops the pair's edge ids / centre atoms at that second offset -- for a fixed j the pairs come i-ascending and a
// pair's edges in shift order, i.e. in ascending edge id.  rowptr[j] is the j-major offset of pair (first atom, j).
// Distances use the host builder's fp64 expression with contraction disabled; the square root is only evaluated for the pairs within 1e-15
// (relative) of the cutoff, which leaves the decision bit-identical.
//
// Open and partly periodic structures (matten_graph_prep_pbc; the reference passes pbc to ASE, data/data.py:285-413):
// an open axis generates no image, S_k = 0.  The prologue completes the cell -- every open-axis row is replaced by a
// unit vector orthogonal to the periodic rows, so the inverse exists whenever the periodic vectors are independent --
// and writes frac = 0 and bound = 0 on the open axes.  shift_range(bound = 0, df = 0) has slack = 1e-6 and returns
// lo = (int)ceil(-1e-6) = 0, hi = (int)floor(1e-6) = 0: exactly [0, 0].  The search kernels therefore walk only S_k = 0
// on an open axis and need no knowledge of pbc; T = S @ cell adds 0 * row there, so a non-zero vector on an open axis
// (kept in `cell` for the model) moves nothing.  On a periodic axis k the column inv[:, k] of the completed inverse
// lies in the span of the periodic rows and does not depend on how the open rows were chosen, so frac and bound are
// those of the periodic sub-lattice.  With all three axes periodic the prologue computes what matten_graph_prep does.
//
// Large structures (matten_neighbor_rows_count / _fill): the pair kernels keep 24 bytes per ordered atom pair.  The rows
// kernels give one wave to each centre atom i; lanes take j = j0 + lane over the atoms of i's crystal in chunks of 64
// and call the same candidate step and pair_walk.  The counting pass writes ONE count per atom; the fill pass recomputes
// the lane counts, places a chunk's edges with a wave prefix sum plus a running base, and the edges of i come out
// j-ascending and shift-lexicographic: the canonical order again, with O(N) bookkeeping.  No CSR is emitted on this route.
//
// Larger structures still (matten_neighbor_cells_*): the rows walk tests every atom of the crystal, O(n^2) arithmetic.
// The cells kernels put a cell list in front of the same walk.  Every crystal gets a grid (cells_grid_kernel): along a
// periodic axis floor(1 / (bound_k (1 + 1e-6))) equal bins of frac - floor(frac) -- an edge has |S_k + df_k| < bound_k,
// so its atoms lie in the same or in adjacent bins modulo nb; below three bins the axis is one bin and is searched as
// before, with several images per pair -- and along an open axis bins at least r_cut |inv[:, k]| (1 + 1e-6) wide over
// the crystal's own extent of pos . inv[:, k] (completed cell), without wrap; never more bins than atoms.  Atoms are
// counted per bin, the caller scans, atom ids are scattered bin by bin (vector atomics: the order inside a bin is
// arbitrary).  One wave per centre atom then concatenates its at most 27 neighbouring bins and walks them 64
// candidates at a time with the unchanged shift_range (unreduced frac difference) + pair_walk: the bins only prune
// which j are looked at.  Candidates do not arrive in j order, so the fill pass keeps the (j, count) records of the
// non-empty ones in LDS (CELLS_ROW_CAP per wave) and places a pair's edges behind the counts of the records with a
// smaller j -- pair_walk emits a pair's images in shift order, so no edge is sorted.  A row with more records than
// that takes rows_walk.  The list is bit for bit that of the other two routes, run to run.
#include "common.h"

#pragma clang fp contract(off)

#define MATTEN_SINGULAR_CELL 1e-12   // the host packer's threshold (predict.pack_structures)

namespace {

struct Cry {
    const double* pos;        // [N,3] all crystals concatenated
    const double* cell;       // [B,9] rows = lattice vectors
    const int64_t* ptr;       // [B+1] first atom of each crystal
    const double* frac;       // [N,3] fractional coordinates (matten_graph_prep)
    const double* bound;      // [B,3] r_cut |inv[:, k]|
    const int64_t* pair_ptr;  // [B+1] first pair of each crystal (sum of n^2)
};

__device__ __forceinline__ void unit_cross(double ux, double uy, double uz, double vx, double vy, double vz, double& x,
                                           double& y, double& z) {
    x = uy * vz - uz * vy, y = uz * vx - ux * vz, z = ux * vy - uy * vx;
    const double n = sqrt((x * x + y * y) + z * z);
    x /= n, y /= n, z /= n;
}

// rows r1, r2 := unit vectors orthogonal to row r0 and to each other (r0 is the only periodic row)
__device__ __forceinline__ void complete_two(const double* r0, double* r1, double* r2) {
    const double fx = fabs(r0[0]), fy = fabs(r0[1]), fz = fabs(r0[2]);
    double ex = 0.0, ey = 0.0, ez = 0.0;   // the coordinate axis r0 leans on least
    if (fx <= fy && fx <= fz) ex = 1.0;
    else if (fy <= fz) ey = 1.0;
    else ez = 1.0;
    unit_cross(r0[0], r0[1], r0[2], ex, ey, ez, r1[0], r1[1], r1[2]);
    unit_cross(r0[0], r0[1], r0[2], r1[0], r1[1], r1[2], r2[0], r2[1], r2[2]);
}

// The cell the inverse is taken of (header comment): every open-axis row of m is replaced by a unit vector orthogonal
// to the periodic rows.  Shared by the prologue and by the grid of the cells route.
__device__ __forceinline__ void complete_open_rows(double* m, bool p0, bool p1, bool p2) {
    const int n_per = (int)p0 + (int)p1 + (int)p2;
    if (n_per == 2) {   // the open row: the unit normal of the two periodic ones (cyclic order keeps the handedness)
        const int o = !p0 ? 0 : (!p1 ? 1 : 2);
        const double* u = m + 3 * ((o + 1) % 3);
        const double* v = m + 3 * ((o + 2) % 3);
        unit_cross(u[0], u[1], u[2], v[0], v[1], v[2], m[3 * o], m[3 * o + 1], m[3 * o + 2]);
    } else if (n_per == 1) {
        const int k = p0 ? 0 : (p1 ? 1 : 2);
        complete_two(m + 3 * k, m + 3 * ((k + 1) % 3), m + 3 * ((k + 2) % 3));
    } else if (n_per == 0) {
        for (int k = 0; k < 9; ++k) m[k] = (k % 4 == 0) ? 1.0 : 0.0;
    }
}

// inv[3 r + k] = (m^-1)[r][k] in closed form, det = det m: frac_k = pos . inv[:, k]
__device__ __forceinline__ void cell_inverse(const double* m, double* inv, double& det) {
    const double ax = m[0], ay = m[1], az = m[2], bx = m[3], by = m[4], bz = m[5], cx = m[6], cy = m[7], cz = m[8];
    // inv = [b x c, c x a, a x b] (as columns) / det
    const double c0x = by * cz - bz * cy, c0y = bz * cx - bx * cz, c0z = bx * cy - by * cx;
    const double c1x = cy * az - cz * ay, c1y = cz * ax - cx * az, c1z = cx * ay - cy * ax;
    const double c2x = ay * bz - az * by, c2y = az * bx - ax * bz, c2z = ax * by - ay * bx;
    det = (ax * c0x + ay * c0y) + az * c0z;
    inv[0] = c0x / det, inv[3] = c0y / det, inv[6] = c0z / det;   // column 0
    inv[1] = c1x / det, inv[4] = c1y / det, inv[7] = c1z / det;
    inv[2] = c2x / det, inv[5] = c2y / det, inv[8] = c2z / det;
}

// PBC = false: matten_graph_prep (three periodic axes).  PBC = true: matten_graph_prep_pbc (header comment); the cell
// that the model receives (cell_f32) is the caller's, the completed one serves the inverse and nothing else.
template <bool PBC>
__global__ __launch_bounds__(64) void graph_prep_kernel(const double* __restrict__ pos, const double* __restrict__ cell,
                                                        const int64_t* __restrict__ ptr, double r_cut,
                                                        double* __restrict__ frac, double* __restrict__ bound,
                                                        int64_t* __restrict__ batch, float* __restrict__ pos_f32,
                                                        float* __restrict__ cell_f32, const uint8_t* __restrict__ pbc,
                                                        int32_t* __restrict__ singular, int64_t* __restrict__ n_singular) {
    const int64_t b = blockIdx.x;
    const double* cl = cell + 9 * b;
    double m[9];
    for (int k = 0; k < 9; ++k) m[k] = cl[k];
    bool p0 = true, p1 = true, p2 = true;
    if (PBC) {
        p0 = pbc[3 * b] != 0, p1 = pbc[3 * b + 1] != 0, p2 = pbc[3 * b + 2] != 0;
        complete_open_rows(m, p0, p1, p2);
    }
    double inv[9], det;
    cell_inverse(m, inv, det);
    if (PBC) {
        // |det| of the completed cell is the volume / area / length of the periodic sub-lattice: the periodic vectors
        // are dependent (or not finite) when it vanishes.  Such a crystal is searched as if open, so that the image
        // loops stay bounded; the host raises from the flag, which rides on the builder's one read-back.
        const bool bad = (p0 || p1 || p2) && !(fabs(det) > MATTEN_SINGULAR_CELL);
        if (threadIdx.x == 0) {
            singular[b] = bad;
            if (bad) atomicAdd((unsigned long long*)n_singular, 1ull);
        }
        if (bad) p0 = p1 = p2 = false;
    }
    const double i00 = inv[0], i10 = inv[3], i20 = inv[6];   // column 0
    const double i01 = inv[1], i11 = inv[4], i21 = inv[7];
    const double i02 = inv[2], i12 = inv[5], i22 = inv[8];
    if (threadIdx.x < 9) cell_f32[9 * b + threadIdx.x] = (float)cl[threadIdx.x];
    if (threadIdx.x == 0) {
        bound[3 * b] = p0 ? r_cut * sqrt((i00 * i00 + i10 * i10) + i20 * i20) : 0.0;
        bound[3 * b + 1] = p1 ? r_cut * sqrt((i01 * i01 + i11 * i11) + i21 * i21) : 0.0;
        bound[3 * b + 2] = p2 ? r_cut * sqrt((i02 * i02 + i12 * i12) + i22 * i22) : 0.0;
    }
    const int64_t lo = ptr[b], hi = ptr[b + 1];
    for (int64_t n = lo + threadIdx.x; n < hi; n += blockDim.x) {
        const double x = pos[3 * n], y = pos[3 * n + 1], z = pos[3 * n + 2];
        frac[3 * n] = p0 ? (x * i00 + y * i10) + z * i20 : 0.0;
        frac[3 * n + 1] = p1 ? (x * i01 + y * i11) + z * i21 : 0.0;
        frac[3 * n + 2] = p2 ? (x * i02 + y * i12) + z * i22 : 0.0;
        pos_f32[3 * n] = (float)x, pos_f32[3 * n + 1] = (float)y, pos_f32[3 * n + 2] = (float)z;
        batch[n] = b;
    }
}

// image shifts along one axis that can hold a neighbour of the pair: [lo, hi] (empty when lo > hi)
__device__ __forceinline__ void shift_range(double bound, double df, int& lo, int& hi) {
    const double slack = 1e-6 * (1.0 + fabs(df) + bound);
    lo = (int)ceil(-bound - df - slack);
    hi = (int)floor(bound - df + slack);
}

// What every route knows of the candidate j of a centre atom i before the distance test: the image shifts that can hold
// a neighbour, and j's position.  A lane without a candidate (live = false) gets empty ranges, so that it walks nothing
// and still takes part in the wave's shuffles.  fi: frac of atom i; bx, by, bz: bound of their crystal.
struct Cand {
    int x0, x1, y0, y1, z0, z1;
    double pj[3];
};

__device__ __forceinline__ Cand candidate(const double* frac, const double* pos, double bx, double by, double bz,
                                          const double* fi, int64_t j, bool live) {
    Cand cd{0, -1, 0, -1, 0, -1, {0.0, 0.0, 0.0}};
    if (live) {
        shift_range(bx, frac[3 * j] - fi[0], cd.x0, cd.x1);
        shift_range(by, frac[3 * j + 1] - fi[1], cd.y0, cd.y1);
        shift_range(bz, frac[3 * j + 2] - fi[2], cd.z0, cd.z1);
        cd.pj[0] = pos[3 * j], cd.pj[1] = pos[3 * j + 1], cd.pj[2] = pos[3 * j + 2];
    }
    return cd;
}

// The distance test of the search, shared by every route so that their decisions cannot diverge: walks the shifts
// [x0,x1] x [y0,y1] x [z0,z1] of one ordered pair in lexicographic order, calls emit(sx, sy, sz) for every edge and
// returns their number.  `self`: i == j, whose zero shift is no edge.
template <class Emit>
__device__ __forceinline__ int pair_walk(const double* __restrict__ cl, const Cand& cd, const double* pi, double r_cut,
                                         bool self, Emit&& emit) {
    const double* pj = cd.pj;
    const double r2 = r_cut * r_cut;
    const double r2_in = r2 * (1.0 - 1e-15), r2_out = r2 * (1.0 + 1e-15);
    int cnt = 0;
    for (int sx = cd.x0; sx <= cd.x1; ++sx)
        for (int sy = cd.y0; sy <= cd.y1; ++sy) {
            // T = S @ cell : ((sx*c0 + sy*c1) + sz*c2) per component, as the host builder's matmul
            const double ax = (double)sx * cl[0] + (double)sy * cl[3];
            const double ay = (double)sx * cl[1] + (double)sy * cl[4];
            const double az = (double)sx * cl[2] + (double)sy * cl[5];
            for (int sz = cd.z0; sz <= cd.z1; ++sz) {
                const double tx = ax + (double)sz * cl[6];
                const double ty = ay + (double)sz * cl[7];
                const double tz = az + (double)sz * cl[8];
                const double dx = (pj[0] + tx) - pi[0], dy = (pj[1] + ty) - pi[1], dz = (pj[2] + tz) - pi[2];
                const double d2 = (dx * dx + dy * dy) + dz * dz;
                bool hit = d2 < r2_in;
                if (!hit && d2 <= r2_out) hit = sqrt(d2) < r_cut;  // the reference's test, needed only at the boundary
                if (hit && !(self && sx == 0 && sy == 0 && sz == 0)) {
                    emit(sx, sy, sz);
                    ++cnt;
                }
            }
        }
    return cnt;
}

struct CsrOut {                // optional outputs of the fill pass: the destination-sorted view (all or none)
    const int64_t* offsets_t;  // [n_pairs + 1] scan of the j-major counts; offsets_t[0] (any constant) is subtracted
    int32_t* rowptr;           // [N + 1]
    int32_t* src_sorted;       // [E] centre atom i of the edge at each sorted position
    int32_t* perm;             // [E] sorted position -> edge id
    int64_t n_atoms;
};

__device__ __forceinline__ void write_edge(int64_t* edge_index, int64_t row_stride, float* shifts, int64_t out, int64_t i,
                                           int64_t j, int sx, int sy, int sz) {
    edge_index[out] = i;
    edge_index[row_stride + out] = j;
    shifts[3 * out] = (float)sx;
    shifts[3 * out + 1] = (float)sy;
    shifts[3 * out + 2] = (float)sz;
}

// PAIR_CAPPED: the fill pass into buffers of fixed capacity (see the capped fill below).  `edge_rows`, the row length of
// edge_index, is then the capacity E_b and the edge count is read from device memory; every store stays behind that
// count, the CSR is always written, and rowptr's closing entry is left to the closing kernel.
enum PairMode { PAIR_COUNT, PAIR_FILL, PAIR_CAPPED };

template <PairMode MODE>
__global__ __launch_bounds__(256) void neighbor_kernel(Cry c, double r_cut, int32_t* __restrict__ counts,
                                                       int32_t* __restrict__ counts_t,
                                                       const int64_t* __restrict__ offsets,
                                                       int64_t* __restrict__ edge_index, int64_t edge_rows,
                                                       float* __restrict__ shifts, float* __restrict__ num_neigh,
                                                       CsrOut csr) {
    constexpr bool FILL = MODE != PAIR_COUNT, CAPPED = MODE == PAIR_CAPPED;
    const int64_t n_edges = CAPPED ? offsets[c.pair_ptr[gridDim.y]] : edge_rows;   // (gridDim.y crystals)
    if (CAPPED && n_edges > edge_rows) return;   // overflow: nothing is stored (the flag is the closing kernel's)
    const int64_t b = blockIdx.y;
    const int64_t lo = c.ptr[b];
    const int64_t n = c.ptr[b + 1] - lo;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * n) return;
    const int64_t i = lo + t / n, j = lo + t % n;
    if (CAPPED && (i >= csr.n_atoms || j >= csr.n_atoms)) return;
    const int64_t pair = c.pair_ptr[b] + t;
    const double* cl = c.cell + 9 * b;
    const double fi[3] = {c.frac[3 * i], c.frac[3 * i + 1], c.frac[3 * i + 2]};
    const Cand cd = candidate(c.frac, c.pos, c.bound[3 * b], c.bound[3 * b + 1], c.bound[3 * b + 2], fi, j, true);
    const double pi[3] = {c.pos[3 * i], c.pos[3 * i + 1], c.pos[3 * i + 2]};
    int64_t out = FILL ? offsets[pair] : 0;
    if (FILL && (CAPPED || num_neigh) && j == lo) num_neigh[i] = (float)(offsets[pair + n] - offsets[pair]);   // i's n pairs
    const int64_t pair_t = c.pair_ptr[b] + (j - lo) * n + (i - lo);   // the same pair numbered j-major
    const bool want_csr = FILL && (CAPPED || csr.rowptr);
    int64_t out_t = 0;
    if (want_csr) {
        out_t = csr.offsets_t[pair_t] - csr.offsets_t[0];   // (a scan that continues the i-major one starts at n_edges)
        if (i == lo) csr.rowptr[j] = (int32_t)out_t;
        if (!CAPPED && pair == 0) csr.rowptr[csr.n_atoms] = (int32_t)n_edges;
    }
    const int cnt = pair_walk(cl, cd, pi, r_cut, i == j, [&](int sx, int sy, int sz) {
        if (FILL) {
            if (!CAPPED || out < n_edges) write_edge(edge_index, edge_rows, shifts, out, i, j, sx, sy, sz);
            if (want_csr) {
                if (!CAPPED || out_t < n_edges) {
                    csr.perm[out_t] = (int32_t)out;
                    csr.src_sorted[out_t] = (int32_t)i;
                }
                ++out_t;
            }
            ++out;
        }
    });
    if (!FILL) {
        counts[pair] = cnt;
        if (counts_t) counts_t[pair_t] = cnt;
    }
}

// {number of edges, smallest edge count of a crystal} from the scanned pair counts: the one read-back of the builder
__global__ __launch_bounds__(256) void neighbor_summary_kernel(const int64_t* __restrict__ offsets,
                                                               const int64_t* __restrict__ pair_ptr, int64_t n_crystals,
                                                               int64_t* __restrict__ out) {
    __shared__ long long red[256];
    long long m = LLONG_MAX;
    for (int64_t b = threadIdx.x; b < n_crystals; b += blockDim.x)
        m = min(m, (long long)(offsets[pair_ptr[b + 1]] - offsets[pair_ptr[b]]));
    red[threadIdx.x] = m;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) red[threadIdx.x] = min(red[threadIdx.x], red[threadIdx.x + o]);
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        out[0] = offsets[pair_ptr[n_crystals]];
        out[1] = n_crystals > 0 ? (int64_t)red[0] : 0;
    }
}

// ---- rows route: one wave per centre atom (header comment) ----
struct Rows {
    const double* pos;      // [N,3]
    const double* cell;     // [B,9]
    const int64_t* ptr;     // [B+1]
    const int64_t* batch;   // [N] crystal of each atom (matten_graph_prep)
    const double* frac;     // [N,3]
    const double* bound;    // [B,3]
    int64_t n_atoms;
};

// inclusive prefix sum of v over the lanes [0, WIDTH) of a wave (WIDTH a power of two; every lane of the wave calls it,
// the lanes from WIDTH on get sums nobody reads)
template <int WIDTH>
__device__ __forceinline__ int wave_inclusive_scan(int v, int lane) {
    for (int off = 1; off < WIDTH; off <<= 1) {
        const int up = __shfl_up(v, off, 64);
        if (lane >= off) v += up;
    }
    return v;
}

// one wave, centre atom i (wave-uniform): every atom of i's crystal in j order.  The whole of the rows route, and the
// walk the cells route falls back on for a row that outgrows its record buffer.
template <bool FILL>
__device__ __forceinline__ void rows_walk(const Rows& c, double r_cut, int64_t i, int lane, int32_t* __restrict__ counts,
                                          const int64_t* __restrict__ offsets, int64_t* __restrict__ edge_index,
                                          int64_t n_edges, float* __restrict__ shifts, float* __restrict__ num_neigh) {
    const int64_t b = c.batch[i];
    const int64_t lo = c.ptr[b], hi = c.ptr[b + 1];
    const double* cl = c.cell + 9 * b;
    const double bx = c.bound[3 * b], by = c.bound[3 * b + 1], bz = c.bound[3 * b + 2];
    const double fi[3] = {c.frac[3 * i], c.frac[3 * i + 1], c.frac[3 * i + 2]};
    const double pi[3] = {c.pos[3 * i], c.pos[3 * i + 1], c.pos[3 * i + 2]};
    int64_t base = FILL ? offsets[i] : 0;   // first edge of atom i; advanced chunk by chunk
    if (FILL && num_neigh && lane == 0) num_neigh[i] = (float)(offsets[i + 1] - offsets[i]);
    int total = 0;
    for (int64_t j0 = lo; j0 < hi; j0 += 64) {   // every lane stays in the loop: the prefix sum below needs all 64
        const int64_t j = j0 + lane;
        const Cand cd = candidate(c.frac, c.pos, bx, by, bz, fi, j, j < hi);   // (lanes past the last atom: not live)
        const int cnt = pair_walk(cl, cd, pi, r_cut, i == j, [](int, int, int) {});
        if (!FILL) {
            total += cnt;
            continue;
        }
        const int incl = wave_inclusive_scan<64>(cnt, lane);
        int64_t out = base + (incl - cnt);
        pair_walk(cl, cd, pi, r_cut, i == j, [&](int sx, int sy, int sz) {
            write_edge(edge_index, n_edges, shifts, out++, i, j, sx, sy, sz);
        });
        base += __shfl(incl, 63, 64);
    }
    if (!FILL) {
        for (int off = 32; off > 0; off >>= 1) total += __shfl_down(total, off, 64);
        if (lane == 0) counts[i] = total;
    }
}

template <bool FILL>
__global__ __launch_bounds__(256) void neighbor_rows_kernel(Rows c, double r_cut, int32_t* __restrict__ counts,
                                                            const int64_t* __restrict__ offsets,
                                                            int64_t* __restrict__ edge_index, int64_t n_edges,
                                                            float* __restrict__ shifts, float* __restrict__ num_neigh) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);   // wave-uniform
    if (i >= c.n_atoms) return;
    rows_walk<FILL>(c, r_cut, i, lane, counts, offsets, edge_index, n_edges, shifts, num_neigh);
}

// ---- cells route: the rows walk over the atoms of the neighbouring bins only (header comment) ----
#define CELLS_ROW_CAP 512        // (j, count) records a wave keeps in LDS: 4 KB per wave, 16 KB per block of four waves
#define CELLS_MAX_NB (1 << 20)   // bins along one axis before the cap at the atom count

struct Cells {
    Rows r;
    const int32_t* grid;        // [B,8] bins along each axis, then 1 where the axis is open (no wrap); two unused
    const int64_t* bin_base;    // [B+1] first bin of each crystal
    const int32_t* bin_of;      // [N] bin of each atom, numbered within its crystal, (c0 nb1 + c1) nb2 + c2
    const int32_t* bin_start;   // [bin_base[B] + 1] first slot of each bin
    const int32_t* slot_atom;   // [N] atom ids, bin by bin
};

// bins along a periodic axis: floor(1 / (bound (1 + 1e-6))).  Below three bins the axis collapses to one: with two,
// c - 1 and c + 1 are the same bin and every candidate would be seen twice.  (A bound that is not finite: one bin.)
__device__ __forceinline__ int periodic_bins(double bound) {
    const double q = 1.0 / (bound * (1.0 + 1e-6));
    return q >= 3.0 ? (q < (double)CELLS_MAX_NB ? (int)q : CELLS_MAX_NB) : 1;
}

// bin of the coordinate t, counted in bin widths from the grid's origin, clamped to the grid (NaN: bin 0)
__device__ __forceinline__ int clamp_bin(double t, int nb) { return t >= 1.0 ? (t < (double)nb ? (int)t : nb - 1) : 0; }

// One block per crystal: bins per axis, and for the open axes the coordinate they are laid along.  A periodic axis is
// binned by frac - floor(frac) in nb equal bins; an open axis by u = pos . inv[:, k] of the completed cell, from the
// smallest u of the crystal in bins at least r_cut |inv[:, k]| (1 + 1e-6) wide.  |d . inv[:, k]| < r_cut |inv[:, k]| for
// every edge, so the two atoms of an edge lie in the same or in adjacent bins (modulo nb on a periodic axis).
__global__ __launch_bounds__(256) void cells_grid_kernel(const double* __restrict__ pos, const double* __restrict__ cell,
                                                         const int64_t* __restrict__ ptr, const double* __restrict__ bound,
                                                         const uint8_t* __restrict__ pbc, const int32_t* __restrict__ singular,
                                                         double r_cut, int32_t* __restrict__ grid, double* __restrict__ gridf,
                                                         int64_t* __restrict__ n_bins) {
    __shared__ double red[4][6];
    const int64_t b = blockIdx.x;
    double m[9];
    for (int k = 0; k < 9; ++k) m[k] = cell[9 * b + k];
    bool per[3] = {true, true, true};
    if (pbc) per[0] = pbc[3 * b] != 0, per[1] = pbc[3 * b + 1] != 0, per[2] = pbc[3 * b + 2] != 0;
    if (singular && singular[b]) per[0] = per[1] = per[2] = false;   // searched as if open, as the prologue says
    const bool any_open = !(per[0] && per[1] && per[2]);
    double inv[9], det;
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    const int64_t first = ptr[b], last = ptr[b + 1];
    if (any_open) {   // (block-uniform)
        complete_open_rows(m, per[0], per[1], per[2]);
        cell_inverse(m, inv, det);
        for (int64_t n = first + threadIdx.x; n < last; n += blockDim.x) {
            const double x = pos[3 * n], y = pos[3 * n + 1], z = pos[3 * n + 2];
            for (int k = 0; k < 3; ++k) {
                const double u = (x * inv[k] + y * inv[3 + k]) + z * inv[6 + k];
                lo[k] = fmin(lo[k], u), hi[k] = fmax(hi[k], u);
            }
        }
        for (int k = 0; k < 3; ++k)
            for (int off = 32; off > 0; off >>= 1) {
                lo[k] = fmin(lo[k], __shfl_xor(lo[k], off, 64));
                hi[k] = fmax(hi[k], __shfl_xor(hi[k], off, 64));
            }
        if ((threadIdx.x & 63) == 0)
            for (int k = 0; k < 3; ++k) red[threadIdx.x >> 6][k] = lo[k], red[threadIdx.x >> 6][3 + k] = hi[k];
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    int nb[3], raw[3];
    double width[3] = {0.0, 0.0, 0.0}, origin[3] = {0.0, 0.0, 0.0};
    for (int k = 0; k < 3; ++k) {
        if (per[k]) {
            nb[k] = raw[k] = periodic_bins(bound[3 * b + k]);
            continue;
        }
        for (int w = 0; w < 4; ++w) lo[k] = fmin(lo[k], red[w][k]), hi[k] = fmax(hi[k], red[w][3 + k]);
        width[k] = r_cut * sqrt((inv[k] * inv[k] + inv[3 + k] * inv[3 + k]) + inv[6 + k] * inv[6 + k]) * (1.0 + 1e-6);
        origin[k] = lo[k];
        nb[k] = raw[k] = clamp_bin((hi[k] - lo[k]) / width[k], CELLS_MAX_NB - 1) + 1;   // (no atom, NaN: one bin)
    }
    // O(N) memory: no more bins than atoms.  The axis with the most bins is halved until that holds.
    const int64_t cap = last - first > 1 ? last - first : 1;
    while ((int64_t)nb[0] * nb[1] * nb[2] > cap) {
        const int k = nb[0] >= nb[1] && nb[0] >= nb[2] ? 0 : (nb[1] >= nb[2] ? 1 : 2);
        nb[k] = (nb[k] + 1) / 2;
        if (per[k] && nb[k] < 3) nb[k] = 1;
    }
    for (int k = 0; k < 3; ++k) {
        if (!per[k]) width[k] = width[k] * ((double)raw[k] / (double)nb[k]);   // the raw bins still cover the extent
        grid[8 * b + k] = nb[k];
        grid[8 * b + 3 + k] = per[k] ? 0 : 1;
        double* gf = gridf + 16 * b + 5 * k;
        gf[0] = per[k] ? 0.0 : inv[k], gf[1] = per[k] ? 0.0 : inv[3 + k], gf[2] = per[k] ? 0.0 : inv[6 + k];
        gf[3] = origin[k], gf[4] = width[k];
    }
    grid[8 * b + 6] = grid[8 * b + 7] = 0;
    gridf[16 * b + 15] = 0.0;
    n_bins[b] = (int64_t)nb[0] * nb[1] * nb[2];
}

// SCATTER = false: the bin of every atom, and the number of atoms of every bin (vector atomics).  SCATTER = true, after
// the caller's scan of those numbers: atom ids bin by bin; the order inside a bin is whatever the atomics produce (the
// order of the edges is fixed later, by j), and bin_count is back at zero afterwards.
template <bool SCATTER>
__global__ __launch_bounds__(256) void cells_bin_kernel(const double* __restrict__ pos, const double* __restrict__ frac,
                                                        const int64_t* __restrict__ batch, const int32_t* __restrict__ grid,
                                                        const double* __restrict__ gridf, const int64_t* __restrict__ bin_base,
                                                        int64_t n_atoms, int32_t* __restrict__ bin_of,
                                                        int32_t* __restrict__ bin_count, const int32_t* __restrict__ bin_start,
                                                        int32_t* __restrict__ slot_atom) {
    const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= n_atoms) return;
    const int64_t b = batch[n];
    if (SCATTER) {
        const int64_t gb = bin_base[b] + bin_of[n];
        const int left = atomicSub(&bin_count[gb], 1);
        slot_atom[bin_start[gb] + left - 1] = (int32_t)n;
        return;
    }
    const int32_t* g = grid + 8 * b;
    int c[3];
    for (int k = 0; k < 3; ++k) {
        const double* gf = gridf + 16 * b + 5 * k;
        double t = 0.0;
        if (g[k] == 1) {
        } else if (g[3 + k]) {
            const double u = (pos[3 * n] * gf[0] + pos[3 * n + 1] * gf[1]) + pos[3 * n + 2] * gf[2];
            t = (u - gf[3]) / gf[4];
        } else {
            const double f = frac[3 * n + k];
            t = (f - floor(f)) * (double)g[k];
        }
        c[k] = clamp_bin(t, g[k]);
    }
    const int bin = (c[0] * g[1] + c[1]) * g[2] + c[2];   // (below the crystal's atom count)
    bin_of[n] = bin;
    atomicAdd(&bin_count[bin_base[b] + bin], 1);
}

// the bin at offset o (-1, 0, 1) from bin c along one axis; false where there is none (or it was counted already)
__device__ __forceinline__ bool neighbour_bin(int c, int o, int nb, int open, int& q) {
    q = c + o;
    if (nb == 1) return o == 0;
    if (open) return q >= 0 && q < nb;
    q = q < 0 ? q + nb : (q >= nb ? q - nb : q);   // nb >= 3: three distinct bins
    return true;
}

template <bool FILL>
__global__ __launch_bounds__(256) void neighbor_cells_kernel(Cells c, double r_cut, int32_t* __restrict__ counts,
                                                             const int64_t* __restrict__ offsets,
                                                             int64_t* __restrict__ edge_index, int64_t n_edges,
                                                             float* __restrict__ shifts, float* __restrict__ num_neigh) {
    __shared__ int2 rec_all[FILL ? 4 * CELLS_ROW_CAP : 1];
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);   // wave-uniform
    if (i >= c.r.n_atoms) return;
    const int64_t b = c.r.batch[i];
    const int32_t* g = c.grid + 8 * b;
    const int n0 = g[0], n1 = g[1], n2 = g[2];
    const int bi = c.bin_of[i];
    const int q0 = bi / (n1 * n2), q1 = (bi / n2) % n1, q2 = bi % n2;
    // lanes 0..26: one neighbouring bin each, its first slot and its length; then the running sum of the lengths
    int start = 0, len = 0;
    if (lane < 27) {
        int a0, a1, a2;
        bool ok = neighbour_bin(q0, lane / 9 - 1, n0, g[3], a0);
        ok = neighbour_bin(q1, (lane / 3) % 3 - 1, n1, g[4], a1) && ok;
        ok = neighbour_bin(q2, lane % 3 - 1, n2, g[5], a2) && ok;
        if (ok) {
            const int64_t gb = c.bin_base[b] + ((int64_t)a0 * n1 + a1) * n2 + a2;
            start = c.bin_start[gb];
            len = c.bin_start[gb + 1] - start;
        }
    }
    const int incl = wave_inclusive_scan<32>(len, lane);
    const int n_cand = __shfl(incl, 26, 64);

    const double* cl = c.r.cell + 9 * b;
    const double bx = c.r.bound[3 * b], by = c.r.bound[3 * b + 1], bz = c.r.bound[3 * b + 2];
    const double fi[3] = {c.r.frac[3 * i], c.r.frac[3 * i + 1], c.r.frac[3 * i + 2]};
    const double pi[3] = {c.r.pos[3 * i], c.r.pos[3 * i + 1], c.r.pos[3 * i + 2]};
    int2* rec = rec_all + (FILL ? (threadIdx.x >> 6) * CELLS_ROW_CAP : 0);
    int total = 0, n_rec = 0;
    bool over = false;
    for (int k0 = 0; k0 < n_cand; k0 += 64) {   // candidates k0 + lane of the concatenated bins; all lanes stay in
        const int k = k0 + lane;
        int slot = -1;
        for (int r = 0; r < 27; ++r) {
            const int e = __shfl(incl, r, 64), l = __shfl(len, r, 64), s0 = __shfl(start, r, 64);
            if (k >= e - l && k < e) slot = s0 + (k - (e - l));
        }
        const bool live = slot >= 0;
        const int64_t j = live ? c.slot_atom[slot] : 0;
        const Cand cd = candidate(c.r.frac, c.r.pos, bx, by, bz, fi, j, live);
        const int cnt = pair_walk(cl, cd, pi, r_cut, live && i == j, [](int, int, int) {});
        if (!FILL) {
            total += cnt;
            continue;
        }
        const unsigned long long hit = __ballot(cnt > 0);
        const int n_hit = __popcll(hit);
        if (n_rec + n_hit > CELLS_ROW_CAP) {   // (wave-uniform)
            over = true;
            break;
        }
        if (cnt > 0) rec[n_rec + __popcll(hit & ((1ull << lane) - 1ull))] = make_int2((int)j, cnt);
        n_rec += n_hit;
    }
    if (!FILL) {
        for (int off = 32; off > 0; off >>= 1) total += __shfl_down(total, off, 64);
        if (lane == 0) counts[i] = total;
        return;
    }
    if (over) {   // a row longer than the record buffer: the j-ordered walk over the whole crystal
        rows_walk<true>(c.r, r_cut, i, lane, nullptr, offsets, edge_index, n_edges, shifts, num_neigh);
        return;
    }
    if (num_neigh && lane == 0) num_neigh[i] = (float)(offsets[i + 1] - offsets[i]);
    // the records are visible to the wave: LDS is in order per wave, the fences keep the compiler from moving the reads
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    // pair_walk emits a pair's images in shift order, so a pair's first edge sits behind the edges of the row's pairs
    // with a smaller j: rank the records, no edge is sorted
    const int64_t base = offsets[i];
    for (int r = lane; r < n_rec; r += 64) {
        const int2 me = rec[r];
        int before = 0;
        for (int q = 0; q < n_rec; ++q) {
            const int2 o = rec[q];
            before += o.x < me.x ? o.y : 0;
        }
        const int64_t j = me.x;
        const Cand cd = candidate(c.r.frac, c.r.pos, bx, by, bz, fi, j, true);
        int64_t out = base + before;
        pair_walk(cl, cd, pi, r_cut, i == j, [&](int sx, int sy, int sz) {
            write_edge(edge_index, n_edges, shifts, out++, i, j, sx, sy, sz);
        });
    }
}

}  // namespace

template <bool PBC>
static int prep_launch(const double* pos, const double* cell, const int64_t* ptr, const uint8_t* pbc, int64_t n_crystals,
                       double r_cut, double* frac, double* bound, int64_t* batch, float* pos_f32, float* cell_f32,
                       int32_t* singular, int64_t* n_singular, hipStream_t stream) {
    if (n_crystals < 0 || !(r_cut > 0.0) || n_crystals >= ((int64_t)1 << 31)) return MATTEN_EINVAL;
    if (n_crystals == 0) return MATTEN_OK;
    if (!pos || !cell || !ptr || !frac || !bound || !batch || !pos_f32 || !cell_f32) return MATTEN_EINVAL;
    if (PBC && (!pbc || !singular || !n_singular)) return MATTEN_EINVAL;
    graph_prep_kernel<PBC><<<(unsigned)n_crystals, 64, 0, stream>>>(pos, cell, ptr, r_cut, frac, bound, batch, pos_f32,
                                                                    cell_f32, pbc, singular, n_singular);
    MATTEN_LAUNCH_CHECK();
    return MATTEN_OK;
}

extern "C" int matten_graph_prep(const double* pos, const double* cell, const int64_t* ptr, int64_t n_crystals,
                                 double r_cut, double* frac, double* bound, int64_t* batch, float* pos_f32,
                                 float* cell_f32, matten_stream_t stream) {
    return prep_launch<false>(pos, cell, ptr, nullptr, n_crystals, r_cut, frac, bound, batch, pos_f32, cell_f32, nullptr,
                              nullptr, (hipStream_t)stream);
}

extern "C" int matten_graph_prep_pbc(const double* pos, const double* cell, const int64_t* ptr, const uint8_t* pbc,
                                     int64_t n_crystals, double r_cut, double* frac, double* bound, int64_t* batch,
                                     float* pos_f32, float* cell_f32, int32_t* singular, int64_t* n_singular,
                                     matten_stream_t stream) {
    return prep_launch<true>(pos, cell, ptr, pbc, n_crystals, r_cut, frac, bound, batch, pos_f32, cell_f32, singular,
                             n_singular, (hipStream_t)stream);
}

// The three entries of the pair search.  n_edges: 0 for the counting pass, the capacity E_b for the capped fill;
// csr_ok: what the entry found of its CSR arguments, which an empty batch does not look at.
template <PairMode MODE>
static int pair_launch(const Cry& c, double r_cut, int64_t n_crystals, int64_t max_atoms, int32_t* counts, int32_t* counts_t,
                       const int64_t* offsets, int64_t n_edges, int64_t* edge_index, float* shifts, float* num_neigh,
                       const CsrOut& csr, bool csr_ok, hipStream_t stream) {
    if (n_crystals < 0 || max_atoms < 0 || n_edges < 0 || !(r_cut > 0.0) || n_crystals > 65535) return MATTEN_EINVAL;
    if (n_crystals == 0 || max_atoms == 0) return MATTEN_OK;
    if (!c.pos || !c.cell || !c.ptr || !c.frac || !c.bound || !c.pair_ptr) return MATTEN_EINVAL;
    if (MODE == PAIR_COUNT ? !counts : !offsets) return MATTEN_EINVAL;
    if ((n_edges > 0 && (!edge_index || !shifts)) || !csr_ok) return MATTEN_EINVAL;
    dim3 grid((unsigned)matten_cdiv(max_atoms * max_atoms, 256), (unsigned)n_crystals);
    neighbor_kernel<MODE><<<grid, 256, 0, stream>>>(c, r_cut, counts, counts_t, offsets, edge_index, n_edges, shifts, num_neigh,
                                                    csr);
    MATTEN_LAUNCH_CHECK();
    return MATTEN_OK;
}

extern "C" int matten_neighbor_count(const double* pos, const double* cell, const int64_t* ptr, const double* frac,
                                     const double* bound, const int64_t* pair_ptr, double r_cut, int64_t n_crystals,
                                     int64_t max_atoms, int32_t* counts, int32_t* counts_t, matten_stream_t stream) {
    return pair_launch<PAIR_COUNT>(Cry{pos, cell, ptr, frac, bound, pair_ptr}, r_cut, n_crystals, max_atoms, counts, counts_t,
                                   nullptr, 0, nullptr, nullptr, nullptr, CsrOut{}, true, (hipStream_t)stream);
}

extern "C" int matten_neighbor_summary(const int64_t* offsets, const int64_t* pair_ptr, int64_t n_crystals,
                                       int64_t* out2, matten_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (n_crystals < 0 || !offsets || !pair_ptr || !out2) return MATTEN_EINVAL;
    neighbor_summary_kernel<<<1, 256, 0, stream>>>(offsets, pair_ptr, n_crystals, out2);
    MATTEN_LAUNCH_CHECK();
    return MATTEN_OK;
}

extern "C" int matten_neighbor_fill(const double* pos, const double* cell, const int64_t* ptr, const double* frac,
                                    const double* bound, const int64_t* pair_ptr, double r_cut, int64_t n_crystals,
                                    int64_t max_atoms, const int64_t* offsets, int64_t n_edges, int64_t* edge_index,
                                    float* edge_cell_shift, float* num_neigh, const int64_t* offsets_t, int64_t n_atoms,
                                    int32_t* rowptr, int32_t* src_sorted, int32_t* perm, matten_stream_t stream) {
    const bool want_csr = offsets_t || rowptr || src_sorted || perm;
    const bool csr_ok = !want_csr || (offsets_t && rowptr && n_atoms >= 0 && n_edges < ((int64_t)1 << 31) &&
                                      (n_edges <= 0 || (src_sorted && perm)));
    return pair_launch<PAIR_FILL>(Cry{pos, cell, ptr, frac, bound, pair_ptr}, r_cut, n_crystals, max_atoms, nullptr, nullptr,
                                  offsets, n_edges, edge_index, edge_cell_shift, num_neigh,
                                  CsrOut{offsets_t, want_csr ? rowptr : nullptr, src_sorted, perm, n_atoms}, csr_ok,
                                  (hipStream_t)stream);
}

static int rows_args_ok(const double* pos, const double* cell, const int64_t* ptr, const int64_t* batch, const double* frac,
                        const double* bound, double r_cut, int64_t n_atoms) {
    if (n_atoms < 0 || !(r_cut > 0.0) || n_atoms >= ((int64_t)1 << 32)) return 0;
    return n_atoms == 0 || (pos && cell && ptr && batch && frac && bound);
}

// The count (FILL = false: counts) and fill entries of the rows and of the cells route: one wave per centre atom.
// args_ok: rows_args_ok / cells_args_ok of the route's inputs `c`.
template <bool FILL, class Kernel, class Args>
static int atom_rows_launch(Kernel kernel, const Args& c, bool args_ok, double r_cut, int64_t n_atoms, int32_t* counts,
                            const int64_t* offsets, int64_t n_edges, int64_t* edge_index, float* shifts, float* num_neigh,
                            hipStream_t stream) {
    if (!args_ok || n_edges < 0) return MATTEN_EINVAL;
    if (n_atoms == 0) return MATTEN_OK;
    if (FILL ? (!offsets || (n_edges > 0 && (!edge_index || !shifts))) : !counts) return MATTEN_EINVAL;
    kernel<<<(unsigned)matten_cdiv(n_atoms, 4), 256, 0, stream>>>(c, r_cut, counts, offsets, edge_index, n_edges, shifts,
                                                                  num_neigh);
    MATTEN_LAUNCH_CHECK();
    return MATTEN_OK;
}

extern "C" int matten_neighbor_rows_count(const double* pos, const double* cell, const int64_t* ptr, const int64_t* batch,
                                          const double* frac, const double* bound, double r_cut, int64_t n_atoms,
                                          int32_t* counts, matten_stream_t stream) {
    return atom_rows_launch<false>(neighbor_rows_kernel<false>, Rows{pos, cell, ptr, batch, frac, bound, n_atoms},
                                   rows_args_ok(pos, cell, ptr, batch, frac, bound, r_cut, n_atoms), r_cut, n_atoms, counts,
                                   nullptr, 0, nullptr, nullptr, nullptr, (hipStream_t)stream);
}

extern "C" int matten_neighbor_rows_fill(const double* pos, const double* cell, const int64_t* ptr, const int64_t* batch,
                                         const double* frac, const double* bound, double r_cut, int64_t n_atoms,
                                         const int64_t* offsets, int64_t n_edges, int64_t* edge_index,
                                         float* edge_cell_shift, float* num_neigh, matten_stream_t stream) {
    return atom_rows_launch<true>(neighbor_rows_kernel<true>, Rows{pos, cell, ptr, batch, frac, bound, n_atoms},
                                  rows_args_ok(pos, cell, ptr, batch, frac, bound, r_cut, n_atoms), r_cut, n_atoms, nullptr,
                                  offsets, n_edges, edge_index, edge_cell_shift, num_neigh, (hipStream_t)stream);
}

extern "C" int matten_neighbor_cells_row_capacity(void) { return CELLS_ROW_CAP; }
extern "C" int matten_neighbor_cells_max_axis_bins(void) { return CELLS_MAX_NB; }

extern "C" int matten_neighbor_cells_grid(const double* pos, const double* cell, const int64_t* ptr, const double* bound,
                                          const uint8_t* pbc, const int32_t* singular, int64_t n_crystals, double r_cut,
                                          int32_t* grid, double* grid_f64, int64_t* n_bins, matten_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (n_crystals < 0 || !(r_cut > 0.0) || n_crystals >= ((int64_t)1 << 31)) return MATTEN_EINVAL;
    if (n_crystals == 0) return MATTEN_OK;
    if (!pos || !cell || !ptr || !bound || !grid || !grid_f64 || !n_bins) return MATTEN_EINVAL;
    cells_grid_kernel<<<(unsigned)n_crystals, 256, 0, stream>>>(pos, cell, ptr, bound, pbc, singular, r_cut, grid, grid_f64,
                                                                n_bins);
    MATTEN_LAUNCH_CHECK();
    return MATTEN_OK;
}

// the cells route numbers atoms and bins in int32
static int cells_args_ok(const double* pos, const double* cell, const int64_t* ptr, const int64_t* batch, const double* frac,
                         const double* bound, double r_cut, int64_t n_atoms, const int32_t* grid, const int64_t* bin_base,
                         const int32_t* bin_of, const int32_t* bin_start, const int32_t* slot_atom) {
    if (!rows_args_ok(pos, cell, ptr, batch, frac, bound, r_cut, n_atoms) || n_atoms >= ((int64_t)1 << 31)) return 0;
    return n_atoms == 0 || (grid && bin_base && bin_of && bin_start && slot_atom);
}

extern "C" int matten_neighbor_cells_bin(const double* pos, const double* frac, const int64_t* batch, const int32_t* grid,
                                         const double* grid_f64, const int64_t* bin_base, int64_t n_atoms, int32_t* bin_of,
                                         int32_t* bin_count, matten_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (n_atoms < 0 || n_atoms >= ((int64_t)1 << 31)) return MATTEN_EINVAL;
    if (n_atoms == 0) return MATTEN_OK;
    if (!pos || !frac || !batch || !grid || !grid_f64 || !bin_base || !bin_of || !bin_count) return MATTEN_EINVAL;
    cells_bin_kernel<false><<<(unsigned)matten_cdiv(n_atoms, 256), 256, 0, stream>>>(pos, frac, batch, grid, grid_f64, bin_base,
                                                                                   n_atoms, bin_of, bin_count, nullptr, nullptr);
    MATTEN_LAUNCH_CHECK();
    return MATTEN_OK;
}

extern "C" int matten_neighbor_cells_scatter(const int64_t* batch, const int64_t* bin_base, const int32_t* bin_of,
                                             const int32_t* bin_start, int64_t n_atoms, int32_t* bin_count,
                                             int32_t* slot_atom, matten_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (n_atoms < 0 || n_atoms >= ((int64_t)1 << 31)) return MATTEN_EINVAL;
    if (n_atoms == 0) return MATTEN_OK;
    if (!batch || !bin_base || !bin_of || !bin_start || !bin_count || !slot_atom) return MATTEN_EINVAL;
    cells_bin_kernel<true><<<(unsigned)matten_cdiv(n_atoms, 256), 256, 0, stream>>>(
        nullptr, nullptr, batch, nullptr, nullptr, bin_base, n_atoms, const_cast<int32_t*>(bin_of), bin_count, bin_start, slot_atom);
    MATTEN_LAUNCH_CHECK();
    return MATTEN_OK;
}

extern "C" int matten_neighbor_cells_count(const double* pos, const double* cell, const int64_t* ptr, const int64_t* batch,
                                           const double* frac, const double* bound, const int32_t* grid,
                                           const int64_t* bin_base, const int32_t* bin_of, const int32_t* bin_start,
                                           const int32_t* slot_atom, double r_cut, int64_t n_atoms, int32_t* counts,
                                           matten_stream_t stream) {
    return atom_rows_launch<false>(
        neighbor_cells_kernel<false>,
        Cells{Rows{pos, cell, ptr, batch, frac, bound, n_atoms}, grid, bin_base, bin_of, bin_start, slot_atom},
        cells_args_ok(pos, cell, ptr, batch, frac, bound, r_cut, n_atoms, grid, bin_base, bin_of, bin_start, slot_atom), r_cut,
        n_atoms, counts, nullptr, 0, nullptr, nullptr, nullptr, (hipStream_t)stream);
}

extern "C" int matten_neighbor_cells_fill(const double* pos, const double* cell, const int64_t* ptr, const int64_t* batch,
                                          const double* frac, const double* bound, const int32_t* grid,
                                          const int64_t* bin_base, const int32_t* bin_of, const int32_t* bin_start,
                                          const int32_t* slot_atom, double r_cut, int64_t n_atoms, const int64_t* offsets,
                                          int64_t n_edges, int64_t* edge_index, float* edge_cell_shift, float* num_neigh,
                                          matten_stream_t stream) {
    return atom_rows_launch<true>(
        neighbor_cells_kernel<true>,
        Cells{Rows{pos, cell, ptr, batch, frac, bound, n_atoms}, grid, bin_base, bin_of, bin_start, slot_atom},
        cells_args_ok(pos, cell, ptr, batch, frac, bound, r_cut, n_atoms, grid, bin_base, bin_of, bin_start, slot_atom), r_cut,
        n_atoms, nullptr, offsets, n_edges, edge_index, edge_cell_shift, num_neigh, (hipStream_t)stream);
}

// ---- capped fill: the pair search into buffers of fixed capacity (N_b, E_b, B_b), edge count read on the device ----
// What a loop over geometries of the same atoms replays as a hipGraph: no host number depends on the positions.  The
// result is the padded batch layout of data/store.py (GraphStoreHost.padded_reference): behind the B real crystals come
// K = B_b - B padding crystals; padding crystal 0 owns P = N_b - N - (K - 1) nodes and all E_b - E padding edges, node q
// of it the edges [floor(q Ep / P), floor((q + 1) Ep / P)), each a self-image edge q -> q with shift (1, 0, 0).  The
// real part is neighbor_kernel<PAIR_CAPPED>'s.  E = offsets[pair_ptr[B]] is read by every thread; when it exceeds E_b no
// thread stores anything but the flag, so the arrays keep the previous, structurally valid list.  Flag bits:
// MATTEN_CAPPED_* (include/matten_hip.h).
namespace {

struct Capped {
    int64_t n_atoms, n_crystals;   // N, B: the real part
    int64_t n_b, e_b, b_b;         // capacities
};

// exclusive scan of int32 counts into int64 offsets[n + 1] by ONE block: a thread sums a contiguous chunk, the chunk
// sums are scanned in LDS, the thread writes its chunk's prefixes.  The capped route serves small cells (a few thousand
// ordered pairs); it replaces the library scan of the eager builder with a launch that is known to capture.
__global__ __launch_bounds__(1024) void neighbor_scan_kernel(const int32_t* __restrict__ counts, int64_t n,
                                                             int64_t* __restrict__ offsets) {
    __shared__ long long part[1024];
    const int64_t chunk = (n + blockDim.x - 1) / blockDim.x;
    const int64_t lo = min(n, (int64_t)threadIdx.x * chunk), hi = min(n, lo + chunk);
    long long s = 0;
    for (int64_t k = lo; k < hi; ++k) s += counts[k];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int o = 1; o < (int)blockDim.x; o <<= 1) {   // Hillis-Steele, inclusive
        const long long v = threadIdx.x >= (unsigned)o ? part[threadIdx.x - o] : 0;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    long long run = part[threadIdx.x] - s;   // exclusive prefix of this chunk
    for (int64_t k = lo; k < hi; ++k) {
        offsets[k] = run;
        run += counts[k];
    }
    if (threadIdx.x == blockDim.x - 1) offsets[n] = part[threadIdx.x];
}

// first padding edge of padding node q: floor(q Ep / P) (q <= P, Ep < 2^31, P < 2^31: exact in int64)
__device__ __forceinline__ int64_t pad_first_edge(int64_t q, int64_t ep, int64_t p) { return q * ep / p; }

// The closing kernel: the flags, and (unless the list overflows) the padding edges, the CSR and the degrees of the padding
// nodes and the valid counts.  One thread per padding edge / padding node, whichever are more.
__global__ __launch_bounds__(256) void neighbor_pad_capped_kernel(const int64_t* __restrict__ offsets,
                                                                  const int64_t* __restrict__ pair_ptr,
                                                                  const int32_t* __restrict__ singular, Capped cap,
                                                                  int64_t* __restrict__ edge_index,
                                                                  float* __restrict__ shifts, float* __restrict__ num_neigh,
                                                                  int32_t* __restrict__ rowptr,
                                                                  int32_t* __restrict__ src_sorted,
                                                                  int32_t* __restrict__ perm, int64_t* __restrict__ n_valid,
                                                                  int32_t* __restrict__ flags) {
    const int64_t n_edges = offsets[pair_ptr[cap.n_crystals]];
    const bool over = n_edges > cap.e_b;
    if (blockIdx.x == 0) {   // the flag word: one block looks at every real crystal, one thread ORs
        int bits = 0;
        for (int64_t b = threadIdx.x; b < cap.n_crystals; b += blockDim.x) {
            if (offsets[pair_ptr[b + 1]] == offsets[pair_ptr[b]]) bits |= MATTEN_CAPPED_EDGELESS;
            if (singular && singular[b]) bits |= MATTEN_CAPPED_SINGULAR;
        }
        const int edgeless = __syncthreads_or(bits & MATTEN_CAPPED_EDGELESS);
        const int sing = __syncthreads_or(bits & MATTEN_CAPPED_SINGULAR);
        if (threadIdx.x == 0) {
            const int word = (over ? MATTEN_CAPPED_OVERFLOW : 0) | (edgeless ? MATTEN_CAPPED_EDGELESS : 0) |
                             (sing ? MATTEN_CAPPED_SINGULAR : 0);
            if (word) flags[0] = flags[0] | word;
            if (!over) n_valid[0] = cap.n_atoms, n_valid[1] = n_edges, n_valid[2] = cap.n_crystals;
        }
    }
    if (over) return;
    const int64_t k = cap.b_b - cap.n_crystals;          // padding crystals
    const int64_t p = cap.n_b - cap.n_atoms - (k - 1);   // nodes of padding crystal 0 (>= 1)
    const int64_t ep = cap.e_b - n_edges;                // padding edges
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < ep) {   // padding edge t: its owner is the last node q with floor(q Ep / P) <= t
        const int64_t q = ((t + 1) * p - 1) / ep;
        const int64_t e = n_edges + t, node = cap.n_atoms + q;
        edge_index[e] = node;
        edge_index[cap.e_b + e] = node;
        shifts[3 * e] = 1.0f, shifts[3 * e + 1] = 0.0f, shifts[3 * e + 2] = 0.0f;
        perm[e] = (int32_t)e;
        src_sorted[e] = (int32_t)node;
    }
    if (t <= cap.n_b - cap.n_atoms) {   // padding node t (t == N_b - N: the closing entry of rowptr)
        const int64_t first = t < p ? n_edges + pad_first_edge(t, ep, p) : cap.e_b;
        rowptr[cap.n_atoms + t] = (int32_t)first;
        if (t < cap.n_b - cap.n_atoms)
            num_neigh[cap.n_atoms + t] = t < p ? (float)(pad_first_edge(t + 1, ep, p) - pad_first_edge(t, ep, p)) : 0.0f;
    }
}

}  // namespace

extern "C" int matten_neighbor_scan(const int32_t* counts, int64_t n, int64_t* offsets, matten_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (n < 0 || !offsets || (n > 0 && !counts)) return MATTEN_EINVAL;
    neighbor_scan_kernel<<<1, 1024, 0, stream>>>(counts, n, offsets);
    MATTEN_LAUNCH_CHECK();
    return MATTEN_OK;
}

extern "C" int matten_neighbor_fill_capped(const double* pos, const double* cell, const int64_t* ptr, const double* frac,
                                           const double* bound, const int64_t* pair_ptr, double r_cut, int64_t n_crystals,
                                           int64_t max_atoms, const int64_t* offsets, const int64_t* offsets_t,
                                           int64_t n_atoms, const int32_t* singular, int64_t node_capacity,
                                           int64_t edge_capacity, int64_t crystal_capacity, int64_t* edge_index,
                                           float* edge_cell_shift, float* num_neigh, int32_t* rowptr, int32_t* src_sorted,
                                           int32_t* perm, int64_t* n_valid, int32_t* flags, matten_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const int64_t lim = (int64_t)1 << 31;
    // pair_launch refuses what matten_neighbor_fill refuses; its empty batches are refused here (a capped batch has atoms)
    if (n_crystals <= 0 || max_atoms <= 0 || n_atoms <= 0) return MATTEN_EINVAL;
    if (!offsets_t || !flags || !n_valid) return MATTEN_EINVAL;
    if (node_capacity < 0 || edge_capacity < 0 || crystal_capacity < 0 || node_capacity >= lim || edge_capacity >= lim ||
        crystal_capacity >= lim)
        return MATTEN_EINVAL;
    // (N_b < N + (B_b - B), written so that no sum can leave int64)
    if (crystal_capacity <= n_crystals || n_atoms > node_capacity || node_capacity - n_atoms < crystal_capacity - n_crystals)
        return MATTEN_EINVAL;
    if (!num_neigh || !rowptr) return MATTEN_EINVAL;
    if (edge_capacity > 0 && (!src_sorted || !perm)) return MATTEN_EINVAL;
    const int rc = pair_launch<PAIR_CAPPED>(Cry{pos, cell, ptr, frac, bound, pair_ptr}, r_cut, n_crystals, max_atoms, nullptr,
                                            nullptr, offsets, edge_capacity, edge_index, edge_cell_shift, num_neigh,
                                            CsrOut{offsets_t, rowptr, src_sorted, perm, n_atoms}, true, stream);
    if (rc != MATTEN_OK) return rc;
    Capped cap{n_atoms, n_crystals, node_capacity, edge_capacity, crystal_capacity};
    const int64_t pad_threads = max(edge_capacity, node_capacity - n_atoms + 1);
    neighbor_pad_capped_kernel<<<(unsigned)matten_cdiv(pad_threads, 256), 256, 0, stream>>>(
        offsets, pair_ptr, singular, cap, edge_index, edge_cell_shift, num_neigh, rowptr, src_sorted, perm, n_valid, flags);
    MATTEN_LAUNCH_CHECK();
    return MATTEN_OK;
}
