// Mean loss over the SELECTED rows of a per-atom prediction (reference model/model.py:340-345: preds[atom_selector], then
// the task's MSELoss, model/task.py:238-248), its adjoint, and the sums the mean-absolute-error metric keeps.
//
// The reference indexes with a boolean mask: the output's shape depends on the data, which costs a host read per step and
// cannot be captured.  Here the selector is an int32 word per row (nonzero = selected; the rows a padded batch appends
// are zero), pred and target have the same [n_rows, d] shape, and everything stays on the device:
//   sum   (fp64)  = sum over selected rows and their d columns of (p - t)^2 (kind 0) or |p - t| (kind 1)
//   count (int64) = selected rows
//   loss  (fp32)  = sum / (count * d) rounded once; 0 when count == 0 (the reference's mean over nothing is NaN)
// An unselected row is loaded but never enters the arithmetic (a select, not a multiply by zero): NaN or Inf there
// changes no output bit.  Differences and squares are formed in fp64 from the fp32 inputs.
//
//   A  loss_partial_kernel  the flattened n_rows * d elements in coalesced strides; one (fp64 sum, int64 count) per
//                           workgroup.  A launch of ONE workgroup writes the result words itself.
//   B  loss_combine_kernel  one workgroup adds the partials in index order and writes the result words.
// The number of workgroups is a function of n_rows * d alone and every sum runs in a fixed order (lane: ascending index;
// wave: xor butterfly; workgroup: waves in index order through LDS; partials: ascending), so two calls give the same
// bits.  No floating-point atomics, no allocation, nothing read back: it captures into a hipGraph as it is.
//
// The same kernels serve the VALID rows of a padded crystal batch (matten_valid_loss / _bwd: the crystal-level loss and
// metric of a captured step).  They are templates on the row predicate: `SelectorRows` reads the int32 word, `ValidRows`
// compares the row with clamp(*n_valid, 0, n_rows), a device word every replay refreshes.  The valid-rows forward keeps
// the squared AND the absolute sum in one pass (the loss and the mean-absolute-error metric of a step); each of them takes
// exactly the additions the one-kind kernel takes, so with selector[row] = (row < *n_valid) the two entries agree bit
// for bit.
#include "common.h"

namespace {

constexpr int SL_THREADS = 256;
constexpr int SL_UNROLL = 4;                         // independent loads in flight per lane
constexpr int SL_TILE = SL_THREADS * SL_UNROLL;      // elements one workgroup takes per round
constexpr int SL_MAX_BLOCKS = 128;                   // above SL_TILE * SL_MAX_BLOCKS elements the workgroups stride

inline int64_t selected_blocks(int64_t n) {
    const int64_t b = (n + SL_TILE - 1) / SL_TILE;
    return b < 1 ? 1 : (b > SL_MAX_BLOCKS ? SL_MAX_BLOCKS : b);
}

template <int KIND>
__device__ __forceinline__ double elem_loss(float p, float t) {
    const double x = (double)p - (double)t;
    return KIND == 0 ? x * x : fabs(x);
}

__device__ __forceinline__ void write_result(double sum, int64_t count, int d, double* __restrict__ out_sum,
                                             int64_t* __restrict__ out_count, float* __restrict__ out_loss) {
    out_sum[0] = sum;
    out_count[0] = count;
    out_loss[0] = count > 0 ? (float)(sum / ((double)count * (double)d)) : 0.0f;
}

// sums over the workgroup, valid in thread 0: butterfly inside each 64-wide wave, then the waves in index order.  Each of
// the NS sums takes exactly the additions a lone one takes.
template <int THREADS, int NS>
__device__ __forceinline__ void block_sum_ordered(double (&x)[NS], int& c, double (*lds_x)[THREADS / 64], int* lds_c) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
        for (int q = 0; q < NS; ++q) x[q] += __shfl_xor(x[q], off, 64);
        c += __shfl_xor(c, off, 64);
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int q = 0; q < NS; ++q) lds_x[q][wave] = x[q];
        lds_c[wave] = c;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int k = 0;
        for (int w = 0; w < THREADS / 64; ++w) k += lds_c[w];
        c = k;
#pragma unroll
        for (int q = 0; q < NS; ++q) {
            double s = 0.0;
            for (int w = 0; w < THREADS / 64; ++w) s += lds_x[q][w];
            x[q] = s;
        }
    }
}

// The row predicates.  `begin` runs once per thread before the first row is asked for.
struct SelectorRows {   // a row counts when its int32 selector word is nonzero
    const int32_t* __restrict__ selector;
    __device__ __forceinline__ void begin() {}
    __device__ __forceinline__ bool operator()(uint32_t row) const { return selector[row] != 0; }
};
struct ValidRows {      // the rows [0, clamp(*n_valid, 0, n_rows)) of a padded crystal batch
    const int64_t* __restrict__ n_valid;
    uint32_t n_rows;
    uint32_t k;
    __device__ __forceinline__ void begin() {
        const int64_t v = n_valid[0];
        k = v < 0 ? 0u : (v > (int64_t)n_rows ? n_rows : (uint32_t)v);
    }
    __device__ __forceinline__ bool operator()(uint32_t row) const { return row < k; }
};

// What a forward produces.  SUMS == one kind (0 or 1): that kind's sum, the selected-loss entry.  SUMS == SL_BOTH: the
// squared and the absolute sum side by side (out_sum[2]) and the loss of the kind `loss_kind` names, the valid-loss entry.
constexpr int SL_BOTH = 2;
template <int SUMS>
struct sums_of {
    static constexpr int NS = SUMS == SL_BOTH ? 2 : 1;
};

template <int NS>
__device__ __forceinline__ void write_results(const double (&sum)[NS], int64_t count, int d, int loss_kind,
                                              double* __restrict__ out_sum, int64_t* __restrict__ out_count,
                                              float* __restrict__ out_loss) {
    const int q = NS == 1 ? 0 : (loss_kind & 1);
    write_result(sum[q], count, d, out_sum + q, out_count, out_loss);
    if (NS > 1) out_sum[1 - q] = sum[1 - q];
}

// n = n_rows * d < 2^31 (checked by the entry): element i belongs to row i / d, and its column-0 element counts the row.
// part_sum holds NS runs of gridDim.x partials, one run per sum.
template <int SUMS, class Rows>
__global__ __launch_bounds__(SL_THREADS) void loss_partial_kernel(const float* __restrict__ pred,
                                                                  const float* __restrict__ target, Rows rows_in, uint32_t n,
                                                                  uint32_t d, int loss_kind, double* __restrict__ part_sum,
                                                                  int64_t* __restrict__ part_count,
                                                                  double* __restrict__ out_sum,
                                                                  int64_t* __restrict__ out_count,
                                                                  float* __restrict__ out_loss) {
    constexpr int NS = sums_of<SUMS>::NS;
    __shared__ double lds_x[NS][SL_THREADS / 64];
    __shared__ int lds_c[SL_THREADS / 64];
    rows_in.begin();
    double acc[NS];
#pragma unroll
    for (int q = 0; q < NS; ++q) acc[q] = 0.0;
    int rows = 0;    // (a lane sees fewer than 2^31 / SL_THREADS elements)
    for (uint64_t base = (uint64_t)blockIdx.x * SL_TILE; base < n; base += (uint64_t)gridDim.x * SL_TILE) {
        float p[SL_UNROLL], t[SL_UNROLL];
        bool s[SL_UNROLL];
        uint32_t col[SL_UNROLL];
#pragma unroll
        for (int u = 0; u < SL_UNROLL; ++u) {
            const uint64_t i = base + (uint64_t)u * SL_THREADS + threadIdx.x;
            p[u] = t[u] = 0.0f, s[u] = false, col[u] = 1;
            if (i < n) {
                const uint32_t row = (uint32_t)i / d;
                col[u] = (uint32_t)i - row * d;
                p[u] = pred[i], t[u] = target[i], s[u] = rows_in(row);
            }
        }
#pragma unroll
        for (int u = 0; u < SL_UNROLL; ++u) {
            if (SUMS == SL_BOTH) {
                const double v0 = elem_loss<0>(p[u], t[u]), v1 = elem_loss<1>(p[u], t[u]);
                acc[0] += s[u] ? v0 : 0.0;
                acc[NS - 1] += s[u] ? v1 : 0.0;
            } else {
                const double v = elem_loss<SUMS>(p[u], t[u]);
                acc[0] += s[u] ? v : 0.0;
            }
            rows += (s[u] && col[u] == 0) ? 1 : 0;
        }
    }
    block_sum_ordered<SL_THREADS, NS>(acc, rows, lds_x, lds_c);
    if (threadIdx.x != 0) return;
    if (gridDim.x == 1) {
        write_results<NS>(acc, (int64_t)rows, (int)d, loss_kind, out_sum, out_count, out_loss);
    } else {
#pragma unroll
        for (int q = 0; q < NS; ++q) part_sum[(size_t)q * gridDim.x + blockIdx.x] = acc[q];
        part_count[blockIdx.x] = (int64_t)rows;
    }
}

template <int NS>
__global__ __launch_bounds__(SL_MAX_BLOCKS) void loss_combine_kernel(const double* __restrict__ part_sum,
                                                                     const int64_t* __restrict__ part_count, int n_partials,
                                                                     int d, int loss_kind, double* __restrict__ out_sum,
                                                                     int64_t* __restrict__ out_count,
                                                                     float* __restrict__ out_loss) {
    __shared__ double lds_x[NS][SL_MAX_BLOCKS];
    __shared__ int64_t lds_c[SL_MAX_BLOCKS];
    const int j = threadIdx.x;
    if (j < n_partials) {   // one parallel fetch, then a fixed order
#pragma unroll
        for (int q = 0; q < NS; ++q) lds_x[q][j] = part_sum[(size_t)q * n_partials + j];
        lds_c[j] = part_count[j];
    }
    __syncthreads();
    if (j != 0) return;
    double s[NS];
    int64_t c = 0;
    for (int k = 0; k < n_partials; ++k) c += lds_c[k];
#pragma unroll
    for (int q = 0; q < NS; ++q) {
        s[q] = 0.0;
        for (int k = 0; k < n_partials; ++k) s[q] += lds_x[q][k];
    }
    write_results<NS>(s, c, d, loss_kind, out_sum, out_count, out_loss);
}

template <int NS>
__global__ void loss_empty_kernel(double* __restrict__ out_sum, int64_t* __restrict__ out_count,
                                  float* __restrict__ out_loss) {
    if (threadIdx.x != 0) return;
    double zero[NS];
#pragma unroll
    for (int q = 0; q < NS; ++q) zero[q] = 0.0;
    write_results<NS>(zero, 0, 1, 0, out_sum, out_count, out_loss);
}

// grad[i] = g * dl(p - t) / (count * d) for the rows of the predicate, +0.0 elsewhere; g and count are device words
template <int KIND, class Rows>
__global__ __launch_bounds__(SL_THREADS) void loss_bwd_kernel(const float* __restrict__ pred,
                                                              const float* __restrict__ target, Rows rows_in, uint32_t n,
                                                              uint32_t d, const float* __restrict__ g,
                                                              const int64_t* __restrict__ count, float* __restrict__ grad) {
    const uint64_t i = (uint64_t)blockIdx.x * SL_THREADS + threadIdx.x;
    if (i >= n) return;
    rows_in.begin();
    const int64_t cnt = count[0];
    const uint32_t row = (uint32_t)i / d;
    const bool sel = cnt > 0 && rows_in(row);
    const double x = (double)pred[i] - (double)target[i];
    double dl;
    if (KIND == 0) dl = 2.0 * x;
    else dl = x > 0.0 ? 1.0 : (x < 0.0 ? -1.0 : (x == 0.0 ? 0.0 : x));   // sign(0) = 0; a NaN stays one
    const double v = (double)g[0] * dl / ((double)cnt * (double)d);
    grad[i] = sel ? (float)v : 0.0f;
}

inline bool selected_bad_shape(int64_t n_rows, int64_t d, int kind) {
    return n_rows < 0 || d < 1 || (kind != 0 && kind != 1) || d >= ((int64_t)1 << 31) ||
           n_rows > (((int64_t)1 << 31) - 1) / d;
}

inline int64_t loss_partials(int64_t n_rows, int64_t d) {   // 0: one workgroup, which writes the results itself
    if (n_rows <= 0 || d < 1 || d >= ((int64_t)1 << 31) || n_rows > (((int64_t)1 << 31) - 1) / d) return 0;
    const int64_t blocks = selected_blocks(n_rows * d);
    return blocks > 1 ? blocks : 0;
}

// the forward of both entries: argument checks that do not concern the predicate, the partial launch, the combine
template <int SUMS, class Rows>
int loss_forward(const float* pred, const float* target, Rows rows, int64_t n_rows, int64_t d, int loss_kind, double* sum,
                 int64_t* count, float* loss, void* workspace, size_t workspace_bytes, hipStream_t stream) {
    constexpr int NS = sums_of<SUMS>::NS;
    const int64_t n = n_rows * d;
    const int blocks = (int)selected_blocks(n);
    const size_t need = (size_t)loss_partials(n_rows, d) * (NS * sizeof(double) + sizeof(int64_t));
    if (need > 0) {
        if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 7)) return MATTEN_EINVAL;
        if (workspace_bytes < need) return MATTEN_ENOMEM;
    }
    double* part_sum = static_cast<double*>(workspace);
    int64_t* part_count = need > 0 ? reinterpret_cast<int64_t*>(part_sum + (size_t)NS * blocks) : nullptr;
    loss_partial_kernel<SUMS, Rows><<<(unsigned)blocks, SL_THREADS, 0, stream>>>(pred, target, rows, (uint32_t)n, (uint32_t)d,
                                                                               loss_kind, part_sum, part_count, sum, count, loss);
    MATTEN_LAUNCH_CHECK();
    if (blocks > 1) {
        loss_combine_kernel<NS><<<1, SL_MAX_BLOCKS, 0, stream>>>(part_sum, part_count, blocks, (int)d, loss_kind, sum, count, loss);
        MATTEN_LAUNCH_CHECK();
    }
    return MATTEN_OK;
}

template <class Rows>
int loss_backward(const float* pred, const float* target, Rows rows, int64_t n_rows, int64_t d, int kind, const float* g,
                  const int64_t* count, float* grad_pred, hipStream_t stream) {
    const int64_t n = n_rows * d;
    const unsigned blocks = (unsigned)matten_cdiv(n, SL_THREADS);
    if (kind == 0)
        loss_bwd_kernel<0, Rows><<<blocks, SL_THREADS, 0, stream>>>(pred, target, rows, (uint32_t)n, (uint32_t)d, g, count, grad_pred);
    else
        loss_bwd_kernel<1, Rows><<<blocks, SL_THREADS, 0, stream>>>(pred, target, rows, (uint32_t)n, (uint32_t)d, g, count, grad_pred);
    MATTEN_LAUNCH_CHECK();
    return MATTEN_OK;
}

}  // namespace

extern "C" int matten_selected_loss_tile_elems(void) { return SL_TILE; }
extern "C" int matten_selected_loss_max_blocks(void) { return SL_MAX_BLOCKS; }

extern "C" size_t matten_selected_loss_workspace_bytes(int64_t n_rows, int64_t d) {
    return (size_t)loss_partials(n_rows, d) * (sizeof(double) + sizeof(int64_t));
}

extern "C" int matten_selected_loss(const float* pred, const float* target, const int32_t* selector, int64_t n_rows,
                                    int64_t d, int kind, double* sum, int64_t* count, float* loss, void* workspace,
                                    size_t workspace_bytes, matten_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (selected_bad_shape(n_rows, d, kind)) return MATTEN_EINVAL;
    if (!sum || !count || !loss) return MATTEN_EINVAL;
    if ((reinterpret_cast<uintptr_t>(sum) | reinterpret_cast<uintptr_t>(count)) & 7) return MATTEN_EINVAL;
    if (n_rows == 0) {
        loss_empty_kernel<1><<<1, 64, 0, stream>>>(sum, count, loss);
        MATTEN_LAUNCH_CHECK();
        return MATTEN_OK;
    }
    if (!pred || !target || !selector) return MATTEN_EINVAL;
    const SelectorRows rows{selector};
    return kind == 0 ? loss_forward<0>(pred, target, rows, n_rows, d, kind, sum, count, loss, workspace, workspace_bytes, stream)
                     : loss_forward<1>(pred, target, rows, n_rows, d, kind, sum, count, loss, workspace, workspace_bytes, stream);
}

extern "C" int matten_selected_loss_bwd(const float* pred, const float* target, const int32_t* selector, int64_t n_rows,
                                        int64_t d, int kind, const float* g, const int64_t* count, float* grad_pred,
                                        matten_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (selected_bad_shape(n_rows, d, kind)) return MATTEN_EINVAL;
    if (!g || !count) return MATTEN_EINVAL;
    if (n_rows == 0) return MATTEN_OK;
    if (!pred || !target || !selector || !grad_pred) return MATTEN_EINVAL;
    return loss_backward(pred, target, SelectorRows{selector}, n_rows, d, kind, g, count, grad_pred, stream);
}

extern "C" size_t matten_valid_loss_workspace_bytes(int64_t n_rows, int64_t d) {
    return (size_t)loss_partials(n_rows, d) * (2 * sizeof(double) + sizeof(int64_t));
}

extern "C" int matten_valid_loss(const float* pred, const float* target, const int64_t* n_valid, int64_t n_rows, int64_t d,
                                 int kind, double* sums, int64_t* count, float* loss, void* workspace,
                                 size_t workspace_bytes, matten_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (selected_bad_shape(n_rows, d, kind)) return MATTEN_EINVAL;
    if (!sums || !count || !loss || !n_valid) return MATTEN_EINVAL;
    if ((reinterpret_cast<uintptr_t>(sums) | reinterpret_cast<uintptr_t>(count) | reinterpret_cast<uintptr_t>(n_valid)) & 7)
        return MATTEN_EINVAL;
    if (n_rows == 0) {
        loss_empty_kernel<2><<<1, 64, 0, stream>>>(sums, count, loss);
        MATTEN_LAUNCH_CHECK();
        return MATTEN_OK;
    }
    if (!pred || !target) return MATTEN_EINVAL;
    return loss_forward<SL_BOTH>(pred, target, ValidRows{n_valid, (uint32_t)n_rows, 0u}, n_rows, d, kind, sums, count, loss,
                                 workspace, workspace_bytes, stream);
}

extern "C" int matten_valid_loss_bwd(const float* pred, const float* target, const int64_t* n_valid, int64_t n_rows,
                                     int64_t d, int kind, const float* g, const int64_t* count, float* grad_pred,
                                     matten_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (selected_bad_shape(n_rows, d, kind)) return MATTEN_EINVAL;
    if (!g || !count || !n_valid || (reinterpret_cast<uintptr_t>(n_valid) & 7)) return MATTEN_EINVAL;
    if (n_rows == 0) return MATTEN_OK;
    if (!pred || !target || !grad_pred) return MATTEN_EINVAL;
    return loss_backward(pred, target, ValidRows{n_valid, (uint32_t)n_rows, 0u}, n_rows, d, kind, g, count, grad_pred, stream);
}
