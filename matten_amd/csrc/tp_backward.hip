// Adjoints of the 'uvu' tensor product + gather + neighbour sum (the most expensive part of a training step), three routes
// over the same forward:
//   matten_tp_backward            table-driven (col_meta / nnz records), per weight column or grouped by input channel: the
//                                 independent second implementation the tests compare the others against
//   matten_tp_backward_lit        dx and dw with the literal-coefficient coupling code of cg_gen.h on a materialised w[E, W]
//   matten_tp_backward_lit_wfree  the same with w re-evaluated per workgroup on the matrix cores
//   matten_tp_backward_sh         dY, the gradient of the edge harmonics
// The last three walk plan.bw_blocks / bw_paths and share the coupling dispatch (for_coupling) and the helpers below it.
#include <type_traits>

#include "cg_gen.h"
#include "common.h"

namespace {

// the forward's normalisation of the messages that arrive at node dst
__device__ __forceinline__ float edge_norm(float avg_nn, const float* __restrict__ num_neigh, int dst) {
    return 1.0f / sqrtf(avg_nn > 0.0f ? avg_nn : num_neigh[dst]);
}

// ------------------------------------------------------------------------------------------------
// 'uvu' TP + gather + scatter, adjoint.  forward (per sorted edge e, weight column q = (path p, u)):
//   agg[dst, out_base + k] += norm(dst) * w[e,q] * sum_ij C_ijk x[src, x_base + i] Y[e, y_off + j]
// backward given G = d agg:
//   dw[e,q]              = norm * sum_{ijk} C_ijk x_i Y_j G[dst, out_base + k]
//   dx[src, x_base + i] += norm * w[e,q] * sum_{jk} C_ijk Y_j G[dst, out_base + k]      (atomic: many edges per src)
// col_meta[W,4]  = {x_base, out_base, nnz_begin, nnz_count | y_off << 16}
// nnz_ijk[nnz,4] = {i, j, k, 0} (uint8), nnz_c[nnz] = sqrt(2 l3+1) C_ijk
// ------------------------------------------------------------------------------------------------
__global__ void tp_backward_kernel(const float* __restrict__ x, int d_in, const void* __restrict__ w_edge, int w_ld,
                                   const float* __restrict__ sh, int sh_stride, const int32_t* __restrict__ src_sorted,
                                   const int32_t* __restrict__ dst_sorted, const int4* __restrict__ col_meta, int W,
                                   const uchar4* __restrict__ nnz_ijk, const float* __restrict__ nnz_c,
                                   const float* __restrict__ g_agg, int d_mid, float avg_nn,
                                   const float* __restrict__ num_neigh, int64_t E, float* __restrict__ dx,
                                   void* __restrict__ dw, int dw_ld, int edge_bf16) {
    int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= E * W) return;
    const int64_t e = idx / W;
    const int q = (int)(idx - e * W);
    const int4 m = col_meta[q];
    const int cnt = m.w & 0xffff, y_off = m.w >> 16;
    const int src = src_sorted[e], dst = dst_sorted[e];
    const float norm = edge_norm(avg_nn, num_neigh, dst);
    const float* xp = x + (int64_t)src * d_in + m.x;
    const float* yp = sh + e * sh_stride + y_off;
    const float* gp = g_agg + (int64_t)dst * d_mid + m.y;
    const float wv = matten_ld_edge(w_edge, e * w_ld + q, edge_bf16);
    float* dxp = dx + (int64_t)src * d_in + m.x;
    const float s = wv * norm;
    // The non-zeros of a coupling are stored i-major (plan.py: np.nonzero order), so the terms of one input component
    // are consecutive: sum them in a scalar and flush per component -- one x load and one atomic per component, no
    // per-term scatter into a register array (that was nine compare / select pairs per term).
    float dwv = 0.0f, acc = 0.0f;
    int cur = cnt > 0 ? (int)nnz_ijk[m.z].x : 0;
    for (int t = 0; t < cnt; ++t) {
        const uchar4 ijk = nnz_ijk[m.z + t];
        const float c = nnz_c[m.z + t];
        if ((int)ijk.x != cur) {
            dwv = fmaf(acc, xp[cur], dwv);
            if (acc != 0.0f) atomicAdd(dxp + cur, s * acc);
            cur = ijk.x;
            acc = 0.0f;
        }
        acc = fmaf(c * yp[ijk.y], gp[ijk.z], acc);
    }
    if (cnt > 0) {
        dwv = fmaf(acc, xp[cur], dwv);
        if (acc != 0.0f) atomicAdd(dxp + cur, s * acc);
    }
    matten_st_edge(dw, e * dw_ld + q, dwv * norm, edge_bf16);
}

// The same adjoint with the weight columns grouped by the INPUT channel they read (in_ptr / in_cols: columns of channel
// c are in_cols[in_ptr[c] .. in_ptr[c+1])): a thread owns (edge, input channel), walks that channel's 5-9 paths and adds
// their contributions to dx in registers, so the gather adjoint costs one atomic per (edge, channel, component)
// instead of one per (edge, path, channel, component).  The atomics were most of the per-column kernel's time
// (~120 M of them per layer at 290 k edges).
__global__ void tp_backward_grouped_kernel(const float* __restrict__ x, int d_in, const void* __restrict__ w_edge, int w_ld,
                                           const float* __restrict__ sh, int sh_stride,
                                           const int32_t* __restrict__ src_sorted, const int32_t* __restrict__ dst_sorted,
                                           const int4* __restrict__ col_meta, const int32_t* __restrict__ in_ptr,
                                           const int32_t* __restrict__ in_cols, int n_in,
                                           const uchar4* __restrict__ nnz_ijk, const float* __restrict__ nnz_c,
                                           const float* __restrict__ g_agg, int d_mid, float avg_nn,
                                           const float* __restrict__ num_neigh, int64_t E, float* __restrict__ dx,
                                           void* __restrict__ dw, int dw_ld, int edge_bf16) {
    int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= E * n_in) return;
    const int64_t e = idx / n_in;
    const int ch = (int)(idx - e * n_in);
    const int src = src_sorted[e], dst = dst_sorted[e];
    const float norm = edge_norm(avg_nn, num_neigh, dst);
    const float* yrow = sh + e * sh_stride;
    const float* grow = g_agg + (int64_t)dst * d_mid;
    float dxi[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) dxi[i] = 0.0f;
    const int c0 = in_ptr[ch], c1 = in_ptr[ch + 1];
    int x_base = 0;
    for (int cc = c0; cc < c1; ++cc) {
        const int q = in_cols[cc];
        const int4 m = col_meta[q];
        const int cnt = m.w & 0xffff;
        x_base = m.x;
        const float* xp = x + (int64_t)src * d_in + m.x;
        const float* yp = yrow + (m.w >> 16);
        const float* gp = grow + m.y;
        const float wv = matten_ld_edge(w_edge, e * w_ld + q, edge_bf16);
        float dwv = 0.0f, acc = 0.0f;
        int cur = cnt > 0 ? (int)nnz_ijk[m.z].x : 0;
        for (int t = 0; t <= cnt; ++t) {   // one extra round flushes the last component
            const bool more = t < cnt;
            const uchar4 ijk = more ? nnz_ijk[m.z + t] : uchar4{255, 0, 0, 0};
            if ((int)ijk.x != cur) {
                dwv = fmaf(acc, xp[cur], dwv);
                const float contrib = wv * acc;
#pragma unroll
                for (int i = 0; i < 9; ++i)
                    if (i == cur) dxi[i] += contrib;
                cur = ijk.x;
                acc = 0.0f;
            }
            if (more) acc = fmaf(nnz_c[m.z + t] * yp[ijk.y], gp[ijk.z], acc);
        }
        matten_st_edge(dw, e * dw_ld + q, dwv * norm, edge_bf16);
    }
    if (c1 > c0) {
        float* dxp = dx + (int64_t)src * d_in + x_base;
#pragma unroll
        for (int i = 0; i < 9; ++i)
            if (dxi[i] != 0.0f) atomicAdd(dxp + i, norm * dxi[i]);
    }
}

}  // namespace

extern "C" int matten_tp_backward(const float* x, int64_t d_in, const void* w_edge, int64_t w_ld, const float* sh_sorted,
                                  int64_t sh_stride, const int32_t* src_sorted, const int32_t* dst_sorted,
                                  const int32_t* col_meta, int64_t n_cols, const uint8_t* nnz_ijk, const float* nnz_c,
                                  const float* g_agg, int64_t d_mid, float avg_num_neighbors, const float* num_neigh,
                                  int64_t n_edges, float* dx /*zero-initialised [N,d_in]*/, void* dw, int64_t dw_ld,
                                  const int32_t* in_ptr, const int32_t* in_cols, int64_t n_in, int edge_is_bf16,
                                  matten_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (n_edges < 0 || d_in <= 0 || n_cols <= 0 || d_mid <= 0 || w_ld < n_cols || dw_ld < n_cols) return MATTEN_EINVAL;
    if (n_edges == 0) return MATTEN_OK;
    if (!x || !w_edge || !sh_sorted || !src_sorted || !dst_sorted || !col_meta || !nnz_ijk || !nnz_c || !g_agg || !dx || !dw)
        return MATTEN_EINVAL;
    if (!(avg_num_neighbors > 0.0f) && !num_neigh) return MATTEN_EINVAL;
    const int T = 256;
    if ((in_ptr == nullptr) != (in_cols == nullptr) || (in_ptr && n_in <= 0)) return MATTEN_EINVAL;
    if (in_ptr) {
        if (matten_cdiv(n_edges * n_in, T) >= ((int64_t)1 << 31)) return MATTEN_EINVAL;
        tp_backward_grouped_kernel<<<(unsigned)matten_cdiv(n_edges * n_in, T), T, 0, stream>>>(
            x, (int)d_in, w_edge, (int)w_ld, sh_sorted, (int)sh_stride, src_sorted, dst_sorted, (const int4*)col_meta,
            in_ptr, in_cols, (int)n_in, (const uchar4*)nnz_ijk, nnz_c, g_agg, (int)d_mid, avg_num_neighbors, num_neigh,
            n_edges, dx, dw, (int)dw_ld, edge_is_bf16);
        MATTEN_LAUNCH_CHECK();
        return MATTEN_OK;
    }
    if (matten_cdiv(n_edges * n_cols, T) >= ((int64_t)1 << 31)) return MATTEN_EINVAL;
    tp_backward_kernel<<<(unsigned)matten_cdiv(n_edges * n_cols, T), T, 0, stream>>>(
        x, (int)d_in, w_edge, (int)w_ld, sh_sorted, (int)sh_stride, src_sorted, dst_sorted, (const int4*)col_meta,
        (int)n_cols, (const uchar4*)nnz_ijk, nnz_c, g_agg, (int)d_mid, avg_num_neighbors, num_neigh, n_edges, dx, dw,
        (int)dw_ld, edge_is_bf16);
    MATTEN_LAUNCH_CHECK();
    return MATTEN_OK;
}

// ------------------------------------------------------------------------------------------------
// 'uvu' TP adjoint with the literal-coefficient coupling code (cg_gen.h CG<l1,l2,l3>::adjoint), the form the forward
// kernels use.  A thread owns (edge, channel u of ONE input block) and walks that block's paths (the list is uniform
// over the block): per path  t_i = sum_jk C_ijk Y_j G_k  (straight-line code, coefficients as literals),
//     dw[e, w_off + u] = norm * sum_i x_i t_i,      dx_i += w * t_i   (registers; ONE atomic per component at the end).
// The table-driven kernels above spend their time fetching (i, j, k, c) records and scattering into dx through compare /
// select chains: 2.14 ms per layer at 294 k edges against 0.28 ms for the forward of the same layer.
// blocks[n_blocks,4] = {x_off, mul, l1, first path | n_paths << 16}; paths[n_paths,4] = {l1*25 + l2*5 + l3, w_off, out_off, 0}
// ------------------------------------------------------------------------------------------------
namespace {

struct LitArgs {
    const float* x;
    const void* w_edge;
    const float* sh;
    const int32_t* src;
    const int32_t* dst;
    const float* g_agg;
    const float* num_neigh;
    float* dx;          // [N, d_in] accumulated with atomics, or (dx_per_edge) [E, d_in]: row e = edge e's contribution
    void* dw;
    int64_t E;
    int d_in, w_ld, sh_stride, d_mid, dw_ld, edge_bf16;
    float avg_nn;
    int dx_per_edge;
};

// The coupling (l2, l3) of an input block of degree L1 from a path's code l1 * 25 + l2 * 5 + l3: f(L2, L3) with both as
// std::integral_constant.  The code is uniform over a block's threads.  LMAX = 2: the instantiations for tensor products
// whose degrees all stay <= 2 (a kernel's registers are those of its widest case: the literal kernel's 60 instead of 108,
// twice the resident waves).  The lists are cg_gen.h's, so a triple the generator knows cannot be missing here.
#define MATTEN_COUPLING_CASE(L1, L2, L3) \
    case (L1 * 25 + L2 * 5 + L3): f(std::integral_constant<int, L2>{}, std::integral_constant<int, L3>{}); break;
template <int L1, int LMAX, class F>
__device__ __forceinline__ void for_coupling(int code, F&& f) {
    if constexpr (LMAX <= 2) {
        if constexpr (L1 == 0) { switch (code) { MATTEN_FOR_EACH_TRIPLE_LE2_L1_0(MATTEN_COUPLING_CASE) default: break; } }
        if constexpr (L1 == 1) { switch (code) { MATTEN_FOR_EACH_TRIPLE_LE2_L1_1(MATTEN_COUPLING_CASE) default: break; } }
        if constexpr (L1 == 2) { switch (code) { MATTEN_FOR_EACH_TRIPLE_LE2_L1_2(MATTEN_COUPLING_CASE) default: break; } }
    } else {
        if constexpr (L1 == 0) { switch (code) { MATTEN_FOR_EACH_TRIPLE_L1_0(MATTEN_COUPLING_CASE) default: break; } }
        if constexpr (L1 == 1) { switch (code) { MATTEN_FOR_EACH_TRIPLE_L1_1(MATTEN_COUPLING_CASE) default: break; } }
        if constexpr (L1 == 2) { switch (code) { MATTEN_FOR_EACH_TRIPLE_L1_2(MATTEN_COUPLING_CASE) default: break; } }
        if constexpr (L1 == 3) { switch (code) { MATTEN_FOR_EACH_TRIPLE_L1_3(MATTEN_COUPLING_CASE) default: break; } }
        if constexpr (L1 == 4) { switch (code) { MATTEN_FOR_EACH_TRIPLE_L1_4(MATTEN_COUPLING_CASE) default: break; } }
    }
}
#undef MATTEN_COUPLING_CASE

// The workgroup's input block b (see tp_backward_lit_kernel for the grid), its lanes per edge and its first workgroup.
// Returned by value, and b rather than blocks[b]: reference parameters and a returned block both moved the kernels' code.
struct BlockAt {
    int b, cu;
    int64_t first;
};
__device__ __forceinline__ BlockAt find_block(const LitArgs& a, const int4* __restrict__ blocks, int n_blocks) {
    int b = 0, cu = 1;
    int64_t first = 0;
    for (;; ++b) {
        cu = 1;
        while (cu < blocks[b].y) cu <<= 1;             // lanes per edge: the block's channels rounded up to a power of two
        const int64_t n = (a.E * cu + 255) / 256;
        if (b + 1 >= n_blocks || (int64_t)blockIdx.x < first + n) break;
        first += n;
    }
    return {b, cu, first};
}

// one (edge, channel u)'s dx contribution to a block at column x_off: into the edge's own row, or its source node's row
template <int D1>
__device__ __forceinline__ void store_dx(const LitArgs& a, int x_off, int64_t e, int src, int u, float norm, const float* __restrict__ dxi) {
    float* dxp = a.dx + (a.dx_per_edge ? e : (int64_t)src) * a.d_in + x_off + u * D1;
#pragma unroll
    for (int i = 0; i < D1; ++i) {
        if (a.dx_per_edge) dxp[i] = norm * dxi[i];   // summed per source node in a fixed order by rows_segment_sum_kernel
        else if (dxi[i] != 0.0f) atomicAdd(dxp + i, norm * dxi[i]);
    }
}

template <int L1, int L2, int L3>
__device__ __forceinline__ void lit_path(const LitArgs& a, const int4 pth, float wv, int64_t e, int u,
                                         const float* __restrict__ x, const float* __restrict__ grow,
                                         const float* __restrict__ yrow, float norm, float* __restrict__ dxi) {
    constexpr int D1 = 2 * L1 + 1, D2 = 2 * L2 + 1, D3 = 2 * L3 + 1;
    float g[D3], y[D2], t[D1];
    const float* gp = grow + pth.z + u * D3;
#pragma unroll
    for (int k = 0; k < D3; ++k) g[k] = gp[k];
#pragma unroll
    for (int j = 0; j < D2; ++j) y[j] = yrow[L2 * L2 + j];
#pragma unroll
    for (int i = 0; i < D1; ++i) t[i] = 0.0f;
    matten::CG<L1, L2, L3>::adjoint(y, g, t);
    float dwv = 0.0f;
#pragma unroll
    for (int i = 0; i < D1; ++i) {
        dwv = fmaf(x[i], t[i], dwv);
        dxi[i] = fmaf(wv, t[i], dxi[i]);
    }
    matten_st_edge(a.dw, e * a.dw_ld + pth.y + u, dwv * norm, a.edge_bf16);
}

// one path of an input block for one (edge, channel): dw written, the edge's dx contribution added into dxi
template <int L1, int LMAX>
__device__ __forceinline__ void lit_one_path(const LitArgs& a, const int4 pth, float wv, int64_t e, int u,
                                             const float* __restrict__ x, const float* __restrict__ grow,
                                             const float* __restrict__ yrow, float norm, float* __restrict__ dxi) {
    for_coupling<L1, LMAX>(pth.x, [&](auto l2, auto l3) {
        lit_path<L1, decltype(l2)::value, decltype(l3)::value>(a, pth, wv, e, u, x, grow, yrow, norm, dxi);
    });
}

template <int L1, int LMAX>
__device__ __forceinline__ void lit_block(const LitArgs& a, const int4 blk, const int4* __restrict__ paths, int64_t e, int u) {
    constexpr int D1 = 2 * L1 + 1;
    const int src = a.src[e], dst = a.dst[e];
    const float norm = edge_norm(a.avg_nn, a.num_neigh, dst);
    const float* xp = a.x + (int64_t)src * a.d_in + blk.x + u * D1;
    float x[D1], dxi[D1];
#pragma unroll
    for (int i = 0; i < D1; ++i) {
        x[i] = xp[i];
        dxi[i] = 0.0f;
    }
    const float* grow = a.g_agg + (int64_t)dst * a.d_mid;
    const float* yrow = a.sh + e * a.sh_stride;
    const int p0 = blk.w & 0xffff, np = blk.w >> 16;
    for (int p = p0; p < p0 + np; ++p) {
        const int4 pth = paths[p];
        const float wv = matten_ld_edge(a.w_edge, e * a.w_ld + pth.y + u, a.edge_bf16);
        lit_one_path<L1, LMAX>(a, pth, wv, e, u, x, grow, yrow, norm, dxi);
    }
    store_dx<D1>(a, blk.x, e, src, u, norm, dxi);
}

// ---- the same adjoint WITHOUT w[E, W] in memory (training on the fused forward) --------------------------------------------
// The workgroup (256 / cu edges x cu channel lanes of one input block) first evaluates the weights it is about to use,
//      w[e, w_off_p + u] = sum_k h2[e, k] W2p[k, w_off_p + u],
// on the matrix cores exactly as the forward does (split fp16: hi hi + 2^-11 (lo hi + hi lo), tp_fused.hip header): per path
// ceil(mul / 16) column tiles of ready-made A fragments (matten_split_a_tiles over pseudo-entries, one per path, REFERENCE
// column order), the edges of the workgroup as the N dimension in tiles of 16, B = the hidden-feature rows h2s[E, 2, 32] the
// forward used.  The D fragments (4 columns of one edge per lane) go to an LDS tile [edge][path][column]; after a barrier
// the (edge, channel) threads run the literal coupling code with w read from there.  Paths are taken in rounds so that
// the tile stays within the launch's LDS (lds_floats); dx accumulates in registers across rounds.  What it saves: matten_radial_mlp in the
// backward (0.36 ms at 293 k edges) and the 4 W bytes per edge of w written and read back; w never exists.
typedef _Float16 wf_f16x8 __attribute__((ext_vector_type(8)));
typedef float wf_f32x4 __attribute__((ext_vector_type(4)));
#ifndef WF_BATCH_N
#define WF_BATCH_N 2
#endif
constexpr int WF_BATCH = WF_BATCH_N;   // matrix jobs of a wave whose operand loads are in flight together
struct WFreeArgs {
    const _Float16* h2s;      // [E, 2, 32]
    const _Float16* frag;     // [n_tiles, 64, 16]: hi(kk 0..7) | lo(kk 0..7) per lane
    const float* w_inv;       // [n_paths] 1 / (the path's fragment scale x the hidden-feature scale)
    int lds_floats;           // capacity of the workgroup's tile (plan.bw_wfree_lds_floats: what the widest block needs, capped)
};

template <int L1, int LMAX>
__device__ __forceinline__ void lit_block_wfree(const LitArgs& a, const WFreeArgs& wf, const int4 blk, const int4* __restrict__ paths,
                                                int cu, int64_t e0, float* __restrict__ wt) {
    constexpr int D1 = 2 * L1 + 1;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 4, c = lane & 15;
    const int epw = 256 / cu;                       // edges of this workgroup
    const int n_et = (epw + 15) >> 4;               // 16-edge MFMA tiles
    const int n_mt = (blk.y + 15) >> 4;             // 16-column tiles per path
    const int tw = (blk.y + 3) & ~3;                // floats of the LDS tile per (edge, path)
    const int p0 = blk.w & 0xffff, np = blk.w >> 16;
    const int per_round = max(1, (wf.lds_floats / epw - 4) / tw);
    const int row = min(np, per_round) * tw + 4;    // floats per edge row of the tile (+4: rows start on different banks)
    // phase-2 role; its edge-invariant loads go out in front of phase 1
    const int el = tid / cu, u = tid & (cu - 1);
    const int64_t e = e0 + el;
    const bool active = e < a.E && u < blk.y;
    int src = 0, dst = 0;
    float norm = 0.0f;
    float x[D1], dxi[D1];
#pragma unroll
    for (int i = 0; i < D1; ++i) x[i] = 0.0f, dxi[i] = 0.0f;
    if (active) {
        src = a.src[e], dst = a.dst[e];
        norm = edge_norm(a.avg_nn, a.num_neigh, dst);
        const float* xp = a.x + (int64_t)src * a.d_in + blk.x + u * D1;
#pragma unroll
        for (int i = 0; i < D1; ++i) x[i] = xp[i];
    }
    const float* grow = a.g_agg + (int64_t)dst * a.d_mid;
    const float* yrow = a.sh + (active ? e : 0) * a.sh_stride;
    const wf_f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    for (int r0 = 0; r0 < np; r0 += per_round) {
        const int nr = min(per_round, np - r0);
        // ---- phase 1: jobs (path, column tile, edge tile) dealt to the four waves in batches of WF_BATCH: all of a batch's
        // operand loads (two 16-byte A pieces per job, the edge tile's two B pieces) go out before the first matrix instruction
        const int n_jobs = nr * n_mt * n_et;
        for (int j0 = wave * WF_BATCH; j0 < n_jobs; j0 += 4 * WF_BATCH) {
            wf_f16x8 ah[WF_BATCH], al[WF_BATCH], bh[WF_BATCH], bl[WF_BATCH];
            float inv[WF_BATCH];
            int dst_off[WF_BATCH];
#pragma unroll
            for (int q = 0; q < WF_BATCH; ++q) {
                const int j = min(j0 + q, n_jobs - 1);
                const int jj = j / n_et, et = j - jj * n_et;
                const int pl = jj / n_mt, mt = jj - pl * n_mt;
                const int4 pth = paths[p0 + r0 + pl];
                const int64_t er = min(e0 + 16 * et + c, a.E - 1);
                const _Float16* fr = wf.frag + ((int64_t)(pth.w + mt) * 64 + lane) * 16;
                ah[q] = *reinterpret_cast<const wf_f16x8*>(fr);
                al[q] = *reinterpret_cast<const wf_f16x8*>(fr + 8);
                bh[q] = *reinterpret_cast<const wf_f16x8*>(wf.h2s + er * 64 + g * 8);
                bl[q] = *reinterpret_cast<const wf_f16x8*>(wf.h2s + er * 64 + 32 + g * 8);
                inv[q] = wf.w_inv[p0 + r0 + pl];
                const int col = 16 * mt + 4 * g;
                dst_off[q] = (j0 + q < n_jobs && 16 * et + c < epw && col < tw) ? (16 * et + c) * row + pl * tw + col : -1;
            }
#pragma unroll
            for (int q = 0; q < WF_BATCH; ++q) {
                wf_f32x4 dl = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[q], bh[q], zero, 0, 0, 0);
                wf_f32x4 dh = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[q], bh[q], zero, 0, 0, 0);
                dl = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[q], bl[q], dl, 0, 0, 0);
                const wf_f32x4 w4 = (dh + (1.0f / 2048.0f) * dl) * inv[q];
                if (dst_off[q] >= 0) *reinterpret_cast<wf_f32x4*>(wt + dst_off[q]) = w4;
            }
        }
        __syncthreads();
        // ---- phase 2: the literal adjoint with w from the tile
        if (active) {
            for (int pl = 0; pl < nr; ++pl) {
                const int4 pth = paths[p0 + r0 + pl];
                lit_one_path<L1, LMAX>(a, pth, wt[el * row + pl * tw + u], e, u, x, grow, yrow, norm, dxi);
            }
        }
        if (r0 + per_round < np) __syncthreads();   // the next round overwrites the tile
    }
    if (active) store_dx<D1>(a, blk.x, e, src, u, norm, dxi);
}

// out[n, c] = sum over k in [ptr[n], ptr[n+1]) of rows[perm[k], c], in k order (fixed: no atomics).  A thread owns one
// column of one segment; two rows are in flight per step (the row index of the step after next is fetched early).
__global__ void rows_segment_sum_kernel(const float* __restrict__ rows, int d, const int32_t* __restrict__ ptr,
                                        const int32_t* __restrict__ perm, int64_t n_seg, float* __restrict__ out) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n_seg * d) return;
    const int64_t n = idx / d;
    const int c = (int)(idx - n * d);
    const int beg = ptr[n], end = ptr[n + 1];
    float acc = 0.0f;
    int k = beg;
    for (; k + 4 <= end; k += 4) {   // four independent loads per step, added in k order
        const float v0 = rows[(int64_t)perm[k] * d + c], v1 = rows[(int64_t)perm[k + 1] * d + c];
        const float v2 = rows[(int64_t)perm[k + 2] * d + c], v3 = rows[(int64_t)perm[k + 3] * d + c];
        acc = (((acc + v0) + v1) + v2) + v3;
    }
    for (; k < end; ++k) acc += rows[(int64_t)perm[k] * d + c];
    out[idx] = acc;
}

// The grid is the input blocks' own workgroup ranges (cdiv(E * lanes per edge, 256) each) laid end to end: a 2-D grid sized
// for the widest block left half of its workgroups without an edge (blocks of 4 channels beside blocks of 32: 100 k
// empty workgroups per launch at 293 k edges).
template <int LMAX>
__global__ __launch_bounds__(256) void tp_backward_lit_kernel(LitArgs a, const int4* __restrict__ blocks, int n_blocks,
                                                              const int4* __restrict__ paths) {
    const auto [b, cu, first] = find_block(a, blocks, n_blocks);
    const int4 blk = blocks[b];
    const int64_t idx = ((int64_t)blockIdx.x - first) * blockDim.x + threadIdx.x;
    const int64_t e = idx / cu;
    const int u = (int)(idx - e * cu);
    if (e >= a.E || u >= blk.y) return;
    switch (blk.z) {
        case 0: lit_block<0, LMAX>(a, blk, paths, e, u); break;
        case 1: lit_block<1, LMAX>(a, blk, paths, e, u); break;
        case 2: lit_block<2, LMAX>(a, blk, paths, e, u); break;
        case 3: if constexpr (LMAX > 2) lit_block<3, LMAX>(a, blk, paths, e, u); break;
        case 4: if constexpr (LMAX > 2) lit_block<4, LMAX>(a, blk, paths, e, u); break;
        default: break;
    }
}

// the same grid as tp_backward_lit_kernel; every thread of a workgroup stays to the end (barriers)
#ifndef WF_MIN_WGS
#define WF_MIN_WGS 6   // l <= 2 instantiation: six workgroups per CU (<= 80 registers; 7 and 8 spill: 1.82 / 2.68 vs 1.53 ms)
#endif
template <int LMAX>
__global__ __launch_bounds__(256, (LMAX <= 2 ? WF_MIN_WGS : 1)) void tp_backward_lit_wfree_kernel(LitArgs a, WFreeArgs wf, const int4* __restrict__ blocks,
                                                                    int n_blocks, const int4* __restrict__ paths) {
    extern __shared__ __attribute__((aligned(16))) float wt[];
    const auto [b, cu, first] = find_block(a, blocks, n_blocks);
    const int4 blk = blocks[b];
    if (cu > 256) return;    // (the entry point refuses max_mul > 256; a table that lies about it computes nothing rather than dividing by zero)
    const int64_t e0 = ((int64_t)blockIdx.x - first) * (256 / cu);
    if (e0 >= a.E) return;   // (workgroup-uniform: the excess workgroups behind the last block)
    switch (blk.z) {
        case 0: lit_block_wfree<0, LMAX>(a, wf, blk, paths, cu, e0, wt); break;
        case 1: lit_block_wfree<1, LMAX>(a, wf, blk, paths, cu, e0, wt); break;
        case 2: lit_block_wfree<2, LMAX>(a, wf, blk, paths, cu, e0, wt); break;
        case 3: if constexpr (LMAX > 2) lit_block_wfree<3, LMAX>(a, wf, blk, paths, cu, e0, wt); break;
        case 4: if constexpr (LMAX > 2) lit_block_wfree<4, LMAX>(a, wf, blk, paths, cu, e0, wt); break;
        default: break;
    }
}
}  // namespace

// The one body of matten_tp_backward_lit (wfree false: w_edge, w_ld) and matten_tp_backward_lit_wfree (wfree true: h2s, frag,
// w_inv, lds_floats, max_mul): the checks, the empty-batch rule, the grid, the LMAX choice and the segment-sum epilogue.
// Where the two routes differ they do so on purpose:
//   sum_lanes    at most 4096 lanes per block on a materialised w, 256 without it: a w-free workgroup is 256 threads =
//                (256 / lanes per edge) edges, so a block wider than 256 channels has no edge per workgroup
//   max_mul      1..256 for the same reason, w-free only (the materialised-w adjoint takes such a layer and needs no width)
//   w_ld         > 0 where there is a w; the w-free entry has no such argument
//   lds_floats   w-free only, 2048..15 * 1024: the narrowest blocks put 256 edges in a workgroup with rows of
//                round4(mul) + 4 floats each (1 channel: 256 x 8), and every block needs at least one path per round
//   operands     with edges, w_edge on the one route, h2s / frag / w_inv on the other
static int tp_backward_lit_launch(bool wfree, const float* x, int64_t d_in, const void* w_edge, int64_t w_ld, const uint16_t* h2s,
                                  const uint16_t* frag, const float* w_inv, const float* sh_sorted, int64_t sh_stride,
                                  const int32_t* src_sorted, const int32_t* dst_sorted, const int32_t* blocks_, int64_t n_blocks,
                                  int64_t sum_lanes, const int32_t* paths_, int64_t n_paths, const float* g_agg, int64_t d_mid,
                                  float avg_num_neighbors, const float* num_neigh, int64_t n_edges, float* dx, void* dw,
                                  int64_t dw_ld, int edge_is_bf16, int64_t n_nodes, const int32_t* out_ptr,
                                  const int32_t* out_perm, float* dx_edges, int64_t lds_floats, int max_l, int max_mul,
                                  matten_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (n_edges < 0 || d_in <= 0 || n_blocks <= 0 || n_blocks > 65535 || n_paths <= 0 || d_mid <= 0 || sum_lanes <= 0 ||
        sum_lanes > (wfree ? 256 : 4096) * n_blocks || dw_ld <= 0)
        return MATTEN_EINVAL;
    if (wfree ? (lds_floats < 2048 || lds_floats > 15 * 1024 || max_mul < 1 || max_mul > 256) : w_ld <= 0) return MATTEN_EINVAL;
    if (dx_edges && (!out_ptr || !out_perm || n_nodes < 0)) return MATTEN_EINVAL;
    if (n_edges == 0) {
        // the fixed-order mode's dx is not initialised by the caller; its dx_edges scratch has no bytes now (a caller may pass
        // NULL for it), so out_ptr marks the mode here (in the atomic mode dx is zero already: zeroing it again is harmless)
        if ((dx_edges || out_ptr) && n_nodes > 0) {
            if (!dx) return MATTEN_EINVAL;
            if (hipMemsetAsync(dx, 0, sizeof(float) * (size_t)n_nodes * (size_t)d_in, stream) != hipSuccess) return MATTEN_ELAUNCH;
        }
        return MATTEN_OK;
    }
    if (!x || !sh_sorted || !src_sorted || !dst_sorted || !blocks_ || !paths_ || !g_agg || !dx || !dw) return MATTEN_EINVAL;
    if (wfree ? (!h2s || !frag || !w_inv) : !w_edge) return MATTEN_EINVAL;
    if (!(avg_num_neighbors > 0.0f) && !num_neigh) return MATTEN_EINVAL;
    // sum_lanes = sum over the blocks of their lanes per edge (channels rounded up to a power of two): the blocks'
    // workgroup ranges laid end to end need at most this many workgroups (the excess ones find no edge and leave)
    const int64_t gx = matten_cdiv(n_edges * sum_lanes, 256) + n_blocks;
    if (gx >= ((int64_t)1 << 31)) return MATTEN_EINVAL;
    const LitArgs a{x, w_edge, sh_sorted, src_sorted, dst_sorted, g_agg, num_neigh, dx_edges ? dx_edges : dx, dw, n_edges,
                   (int)d_in, (int)w_ld, (int)sh_stride, (int)d_mid, (int)dw_ld, edge_is_bf16, avg_num_neighbors, dx_edges ? 1 : 0};
    const WFreeArgs wf{(const _Float16*)h2s, (const _Float16*)frag, w_inv, (int)lds_floats};
    const int4* blocks = (const int4*)blocks_;
    const int4* paths = (const int4*)paths_;
    const size_t lds = sizeof(float) * (size_t)lds_floats;
    if (!wfree && max_l <= 2) tp_backward_lit_kernel<2><<<(unsigned)gx, 256, 0, stream>>>(a, blocks, (int)n_blocks, paths);
    else if (!wfree) tp_backward_lit_kernel<4><<<(unsigned)gx, 256, 0, stream>>>(a, blocks, (int)n_blocks, paths);
    else if (max_l <= 2) tp_backward_lit_wfree_kernel<2><<<(unsigned)gx, 256, lds, stream>>>(a, wf, blocks, (int)n_blocks, paths);
    else tp_backward_lit_wfree_kernel<4><<<(unsigned)gx, 256, lds, stream>>>(a, wf, blocks, (int)n_blocks, paths);
    MATTEN_LAUNCH_CHECK();
    if (dx_edges && n_nodes > 0) {
        if (matten_cdiv(n_nodes * d_in, 256) >= ((int64_t)1 << 31)) return MATTEN_EINVAL;
        rows_segment_sum_kernel<<<(unsigned)matten_cdiv(n_nodes * d_in, 256), 256, 0, stream>>>(dx_edges, (int)d_in, out_ptr,
                                                                                              out_perm, n_nodes, dx);
        MATTEN_LAUNCH_CHECK();
    }
    return MATTEN_OK;
}

extern "C" int matten_tp_backward_lit(const float* x, int64_t d_in, const void* w_edge, int64_t w_ld, const float* sh_sorted,
                                      int64_t sh_stride, const int32_t* src_sorted, const int32_t* dst_sorted,
                                      const int32_t* blocks, int64_t n_blocks, int64_t sum_lanes, const int32_t* paths,
                                      int64_t n_paths, const float* g_agg, int64_t d_mid, float avg_num_neighbors,
                                      const float* num_neigh, int64_t n_edges, float* dx, void* dw, int64_t dw_ld,
                                      int edge_is_bf16, int64_t n_nodes, const int32_t* out_ptr, const int32_t* out_perm,
                                      float* dx_edges, int max_l, matten_stream_t stream_) {
    return tp_backward_lit_launch(false, x, d_in, w_edge, w_ld, nullptr, nullptr, nullptr, sh_sorted, sh_stride, src_sorted,
                                  dst_sorted, blocks, n_blocks, sum_lanes, paths, n_paths, g_agg, d_mid, avg_num_neighbors,
                                  num_neigh, n_edges, dx, dw, dw_ld, edge_is_bf16, n_nodes, out_ptr, out_perm, dx_edges, 0, max_l,
                                  0, stream_);
}

// matten_tp_backward_lit without w[E, W]: the weights are re-evaluated per workgroup on the matrix cores from the hidden
// features (see lit_block_wfree).  paths[p].w = first A-fragment tile of path p; frag / w_inv from matten_split_a_tiles over one
// pseudo-entry per path (words 5, 6, 7 = w_off, first tile, ceil(mul / 16)) on the last radial layer in REFERENCE column order.
extern "C" int matten_tp_backward_lit_wfree(const float* x, int64_t d_in, const uint16_t* h2s, const uint16_t* frag,
                                            const float* w_inv, const float* sh_sorted, int64_t sh_stride,
                                            const int32_t* src_sorted, const int32_t* dst_sorted, const int32_t* blocks,
                                            int64_t n_blocks, int64_t sum_lanes, const int32_t* paths, int64_t n_paths,
                                            const float* g_agg, int64_t d_mid, float avg_num_neighbors, const float* num_neigh,
                                            int64_t n_edges, float* dx, void* dw, int64_t dw_ld, int edge_is_bf16,
                                            int64_t n_nodes, const int32_t* out_ptr, const int32_t* out_perm, float* dx_edges,
                                            int64_t lds_floats, int max_l, int max_mul, matten_stream_t stream_) {
    return tp_backward_lit_launch(true, x, d_in, nullptr, 0, h2s, frag, w_inv, sh_sorted, sh_stride, src_sorted, dst_sorted, blocks,
                                  n_blocks, sum_lanes, paths, n_paths, g_agg, d_mid, avg_num_neighbors, num_neigh, n_edges, dx, dw,
                                  dw_ld, edge_is_bf16, n_nodes, out_ptr, out_perm, dx_edges, lds_floats, max_l, max_mul, stream_);
}

// ------------------------------------------------------------------------------------------------
// 'uvu' TP adjoint w.r.t. the edge harmonics (geometry gradients), the third adjoint beside dx and dw above:
//     dY[e, l2^2 + j] = norm(dst_e) * sum_paths sum_u w[e, w_off + u] * s_j,   s_j = sum_ik C_ijk x_i G_k
// (cg_gen.h CG<l1,l2,l3>::harmonic).  The sum runs over every channel of every input block and every path of ONE edge, so
// a launch row owns the whole edge: `cu` lanes per edge (the widest block's channels rounded up to a power of two, at
// most a wave), 64 / cu edges per wave; a lane takes the channels u = lane, lane + cu, ... of each block in turn and
// keeps (LMAX+1)^2 accumulators across the walk.  One xor-butterfly over the edge's lanes follows (every lane ends with
// the same bits: each step adds the same two numbers on both sides), then the row is stored whole, zeros behind
// (LMAX+1)^2.  No atomics; the same tables as tp_backward_lit_kernel.
// ------------------------------------------------------------------------------------------------
namespace {

// LitArgs without sh, dx and dw, with dy.  Its own struct on purpose: with the fields folded into LitArgs (either order) the
// harmonics kernel's argument loads split up and its l <= 4 instantiation, at 106 scalar registers, spills five more of them.
struct ShArgs {
    const float* x;
    const void* w_edge;
    const int32_t* src;
    const int32_t* dst;
    const float* g_agg;
    const float* num_neigh;
    float* dy;
    int64_t E;
    int d_in, w_ld, sh_stride, d_mid, edge_bf16;
    float avg_nn;
};

template <int L1, int L2, int L3>
__device__ __forceinline__ void sh_path(const int4 pth, float wv, int u, const float* __restrict__ x,
                                        const float* __restrict__ grow, float* __restrict__ acc) {
    constexpr int D2 = 2 * L2 + 1, D3 = 2 * L3 + 1;
    float g[D3], s[D2];
    const float* gp = grow + pth.z + u * D3;
#pragma unroll
    for (int k = 0; k < D3; ++k) g[k] = gp[k];
#pragma unroll
    for (int j = 0; j < D2; ++j) s[j] = 0.0f;
    matten::CG<L1, L2, L3>::harmonic(x, g, s);
#pragma unroll
    for (int j = 0; j < D2; ++j) acc[L2 * L2 + j] = fmaf(wv, s[j], acc[L2 * L2 + j]);
}

// the channels u = lu, lu + cu, ... of one input block for one edge, all of the block's paths
template <int L1, int LMAX>
__device__ __forceinline__ void sh_block(const ShArgs& a, const int4 blk, const int4* __restrict__ paths, int64_t e, int src,
                                         const float* __restrict__ grow, int lu, int cu, float* __restrict__ acc) {
    constexpr int D1 = 2 * L1 + 1;
    const int p0 = blk.w & 0xffff, np = blk.w >> 16;
    for (int u = lu; u < blk.y; u += cu) {
        const float* xp = a.x + (int64_t)src * a.d_in + blk.x + u * D1;
        float x[D1];
#pragma unroll
        for (int i = 0; i < D1; ++i) x[i] = xp[i];
        for (int p = p0; p < p0 + np; ++p) {
            const int4 pth = paths[p];
            const float wv = matten_ld_edge(a.w_edge, e * a.w_ld + pth.y + u, a.edge_bf16);
            for_coupling<L1, LMAX>(pth.x, [&](auto l2, auto l3) {
                sh_path<L1, decltype(l2)::value, decltype(l3)::value>(pth, wv, u, x, grow, acc);
            });
        }
    }
}

template <int LMAX>
__global__ __launch_bounds__(256) void tp_backward_sh_kernel(ShArgs a, const int4* __restrict__ blocks, int n_blocks,
                                                             const int4* __restrict__ paths, int cu) {
    constexpr int SH = (LMAX + 1) * (LMAX + 1);
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t e_raw = idx / cu;
    const int lu = (int)(idx - e_raw * cu);
    // lanes behind the last edge stay for the butterfly (cu divides 64: an edge's lanes share a wave) and add zeros
    const bool live = e_raw < a.E;
    const int64_t e = live ? e_raw : a.E - 1;
    const int src = a.src[e], dst = a.dst[e];
    float acc[SH];
#pragma unroll
    for (int k = 0; k < SH; ++k) acc[k] = 0.0f;
    if (live) {
        const float* grow = a.g_agg + (int64_t)dst * a.d_mid;
        for (int b = 0; b < n_blocks; ++b) {
            const int4 blk = blocks[b];
            switch (blk.z) {   // uniform over the launch
                case 0: sh_block<0, LMAX>(a, blk, paths, e, src, grow, lu, cu, acc); break;
                case 1: sh_block<1, LMAX>(a, blk, paths, e, src, grow, lu, cu, acc); break;
                case 2: sh_block<2, LMAX>(a, blk, paths, e, src, grow, lu, cu, acc); break;
                case 3: if constexpr (LMAX > 2) sh_block<3, LMAX>(a, blk, paths, e, src, grow, lu, cu, acc); break;
                case 4: if constexpr (LMAX > 2) sh_block<4, LMAX>(a, blk, paths, e, src, grow, lu, cu, acc); break;
                default: break;
            }
        }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        if (d < cu) {
#pragma unroll
            for (int k = 0; k < SH; ++k) acc[k] += __shfl_xor(acc[k], d, 64);
        }
    }
    if (!live) return;
    const float norm = edge_norm(a.avg_nn, a.num_neigh, dst);
    float* row = a.dy + e * a.sh_stride;
#pragma unroll
    for (int k = 0; k < SH; ++k)
        if (lu == (k & (cu - 1)) && k < a.sh_stride) row[k] = norm * acc[k];
    for (int k = SH + lu; k < a.sh_stride; k += cu) row[k] = 0.0f;
}
}  // namespace

extern "C" int matten_tp_backward_sh(const float* x, int64_t d_in, const void* w_edge, int64_t w_ld, const int32_t* src_sorted,
                                     const int32_t* dst_sorted, const int32_t* blocks, int64_t n_blocks, int64_t max_mul,
                                     const int32_t* paths, int64_t n_paths, const float* g_agg, int64_t d_mid,
                                     float avg_num_neighbors, const float* num_neigh, int64_t n_edges, int edge_is_bf16,
                                     float* dy, int64_t sh_stride, int max_l, matten_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (n_edges < 0 || d_in <= 0 || n_blocks <= 0 || n_blocks > 65535 || n_paths <= 0 || d_mid <= 0 || max_mul <= 0 ||
        w_ld <= 0 || max_l < 0 || max_l > 4 || sh_stride < (max_l <= 2 ? 9 : 25))
        return MATTEN_EINVAL;
    if (n_edges == 0) return MATTEN_OK;
    if (!x || !w_edge || !src_sorted || !dst_sorted || !blocks || !paths || !g_agg || !dy) return MATTEN_EINVAL;
    if (!(avg_num_neighbors > 0.0f) && !num_neigh) return MATTEN_EINVAL;
    int cu = 1;   // lanes per edge
    while (cu < max_mul && cu < 64) cu <<= 1;
    const int64_t gx = matten_cdiv(n_edges * cu, 256);
    if (gx >= ((int64_t)1 << 31)) return MATTEN_EINVAL;
    ShArgs a{x, w_edge, src_sorted, dst_sorted, g_agg, num_neigh, dy, n_edges, (int)d_in, (int)w_ld, (int)sh_stride, (int)d_mid,
             edge_is_bf16, avg_num_neighbors};
    if (max_l <= 2) tp_backward_sh_kernel<2><<<(unsigned)gx, 256, 0, stream>>>(a, (const int4*)blocks, (int)n_blocks, (const int4*)paths, cu);
    else tp_backward_sh_kernel<4><<<(unsigned)gx, 256, 0, stream>>>(a, (const int4*)blocks, (int)n_blocks, (const int4*)paths, cu);
    MATTEN_LAUNCH_CHECK();
    return MATTEN_OK;
}
