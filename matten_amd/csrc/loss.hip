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
//   A  selected_partial_kernel  the flattened n_rows * d elements in coalesced strides; one (fp64 sum, int64 count) per
//                               workgroup.  A launch of ONE workgroup writes the three result words itself.
//   B  selected_combine_kernel  one workgroup adds the partials in index order and writes the result words.
// The number of workgroups is a function of n_rows * d alone and every sum runs in a fixed order (lane: ascending index;
// wave: xor butterfly; workgroup: waves in index order through LDS; partials: ascending), so two calls give the same
// bits.  No floating-point atomics, no allocation, nothing read back: it captures into a hipGraph as it is.
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

// sums over the workgroup, valid in thread 0: butterfly inside each 64-wide wave, then the waves in index order
template <int THREADS>
__device__ __forceinline__ void block_sum_ordered(double& x, int& c, double* lds_x, int* lds_c) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        x += __shfl_xor(x, off, 64);
        c += __shfl_xor(c, off, 64);
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) lds_x[wave] = x, lds_c[wave] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        int k = 0;
        for (int w = 0; w < THREADS / 64; ++w) s += lds_x[w], k += lds_c[w];
        x = s, c = k;
    }
}

// n = n_rows * d < 2^31 (checked by the entry): element i belongs to row i / d, and its column-0 element counts the row
template <int KIND>
__global__ __launch_bounds__(SL_THREADS) void selected_partial_kernel(const float* __restrict__ pred,
                                                                      const float* __restrict__ target,
                                                                      const int32_t* __restrict__ selector, uint32_t n,
                                                                      uint32_t d, double* __restrict__ part_sum,
                                                                      int64_t* __restrict__ part_count,
                                                                      double* __restrict__ out_sum,
                                                                      int64_t* __restrict__ out_count,
                                                                      float* __restrict__ out_loss) {
    __shared__ double lds_x[SL_THREADS / 64];
    __shared__ int lds_c[SL_THREADS / 64];
    double acc = 0.0;
    int rows = 0;    // (a lane sees fewer than 2^31 / SL_THREADS elements)
    for (uint64_t base = (uint64_t)blockIdx.x * SL_TILE; base < n; base += (uint64_t)gridDim.x * SL_TILE) {
        float p[SL_UNROLL], t[SL_UNROLL];
        int32_t s[SL_UNROLL];
        uint32_t col[SL_UNROLL];
#pragma unroll
        for (int u = 0; u < SL_UNROLL; ++u) {
            const uint64_t i = base + (uint64_t)u * SL_THREADS + threadIdx.x;
            p[u] = t[u] = 0.0f, s[u] = 0, col[u] = 1;
            if (i < n) {
                const uint32_t row = (uint32_t)i / d;
                col[u] = (uint32_t)i - row * d;
                p[u] = pred[i], t[u] = target[i], s[u] = selector[row];
            }
        }
#pragma unroll
        for (int u = 0; u < SL_UNROLL; ++u) {
            const double v = elem_loss<KIND>(p[u], t[u]);
            acc += s[u] != 0 ? v : 0.0;
            rows += (s[u] != 0 && col[u] == 0) ? 1 : 0;
        }
    }
    block_sum_ordered<SL_THREADS>(acc, rows, lds_x, lds_c);
    if (threadIdx.x != 0) return;
    if (gridDim.x == 1) write_result(acc, (int64_t)rows, (int)d, out_sum, out_count, out_loss);
    else part_sum[blockIdx.x] = acc, part_count[blockIdx.x] = (int64_t)rows;
}

__global__ __launch_bounds__(SL_MAX_BLOCKS) void selected_combine_kernel(const double* __restrict__ part_sum,
                                                                         const int64_t* __restrict__ part_count,
                                                                         int n_partials, int d, double* __restrict__ out_sum,
                                                                         int64_t* __restrict__ out_count,
                                                                         float* __restrict__ out_loss) {
    __shared__ double lds_x[SL_MAX_BLOCKS];
    __shared__ int64_t lds_c[SL_MAX_BLOCKS];
    const int j = threadIdx.x;
    if (j < n_partials) lds_x[j] = part_sum[j], lds_c[j] = part_count[j];   // one parallel fetch, then a fixed order
    __syncthreads();
    if (j != 0) return;
    double s = 0.0;
    int64_t c = 0;
    for (int k = 0; k < n_partials; ++k) s += lds_x[k], c += lds_c[k];
    write_result(s, c, d, out_sum, out_count, out_loss);
}

__global__ void selected_empty_kernel(double* __restrict__ out_sum, int64_t* __restrict__ out_count,
                                      float* __restrict__ out_loss) {
    if (threadIdx.x == 0) write_result(0.0, 0, 1, out_sum, out_count, out_loss);
}

// grad[i] = g * dl(p - t) / (count * d) for selected rows, +0.0 elsewhere; g and count are device words
template <int KIND>
__global__ __launch_bounds__(SL_THREADS) void selected_bwd_kernel(const float* __restrict__ pred,
                                                                  const float* __restrict__ target,
                                                                  const int32_t* __restrict__ selector, uint32_t n, uint32_t d,
                                                                  const float* __restrict__ g, const int64_t* __restrict__ count,
                                                                  float* __restrict__ grad) {
    const uint64_t i = (uint64_t)blockIdx.x * SL_THREADS + threadIdx.x;
    if (i >= n) return;
    const int64_t cnt = count[0];
    const uint32_t row = (uint32_t)i / d;
    const bool sel = cnt > 0 && selector[row] != 0;
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

}  // namespace

extern "C" int matten_selected_loss_tile_elems(void) { return SL_TILE; }
extern "C" int matten_selected_loss_max_blocks(void) { return SL_MAX_BLOCKS; }

extern "C" size_t matten_selected_loss_workspace_bytes(int64_t n_rows, int64_t d) {
    if (n_rows <= 0 || d < 1 || d >= ((int64_t)1 << 31) || n_rows > (((int64_t)1 << 31) - 1) / d) return 0;
    const int64_t blocks = selected_blocks(n_rows * d);
    return blocks > 1 ? (size_t)blocks * (sizeof(double) + sizeof(int64_t)) : 0;
}

extern "C" int matten_selected_loss(const float* pred, const float* target, const int32_t* selector, int64_t n_rows,
                                    int64_t d, int kind, double* sum, int64_t* count, float* loss, void* workspace,
                                    size_t workspace_bytes, matten_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (selected_bad_shape(n_rows, d, kind)) return MATTEN_EINVAL;
    if (!sum || !count || !loss) return MATTEN_EINVAL;
    if ((reinterpret_cast<uintptr_t>(sum) | reinterpret_cast<uintptr_t>(count)) & 7) return MATTEN_EINVAL;
    if (n_rows == 0) {
        selected_empty_kernel<<<1, 64, 0, stream>>>(sum, count, loss);
        MATTEN_LAUNCH_CHECK();
        return MATTEN_OK;
    }
    if (!pred || !target || !selector) return MATTEN_EINVAL;
    const int64_t n = n_rows * d;
    const int blocks = (int)selected_blocks(n);
    const size_t need = matten_selected_loss_workspace_bytes(n_rows, d);
    if (need > 0) {
        if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 7)) return MATTEN_EINVAL;
        if (workspace_bytes < need) return MATTEN_ENOMEM;
    }
    double* part_sum = static_cast<double*>(workspace);
    int64_t* part_count = need > 0 ? reinterpret_cast<int64_t*>(part_sum + blocks) : nullptr;
    if (kind == 0)
        selected_partial_kernel<0><<<(unsigned)blocks, SL_THREADS, 0, stream>>>(pred, target, selector, (uint32_t)n, (uint32_t)d,
                                                                                part_sum, part_count, sum, count, loss);
    else
        selected_partial_kernel<1><<<(unsigned)blocks, SL_THREADS, 0, stream>>>(pred, target, selector, (uint32_t)n, (uint32_t)d,
                                                                                part_sum, part_count, sum, count, loss);
    MATTEN_LAUNCH_CHECK();
    if (blocks > 1) {
        selected_combine_kernel<<<1, SL_MAX_BLOCKS, 0, stream>>>(part_sum, part_count, blocks, (int)d, sum, count, loss);
        MATTEN_LAUNCH_CHECK();
    }
    return MATTEN_OK;
}

extern "C" int matten_selected_loss_bwd(const float* pred, const float* target, const int32_t* selector, int64_t n_rows,
                                        int64_t d, int kind, const float* g, const int64_t* count, float* grad_pred,
                                        matten_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (selected_bad_shape(n_rows, d, kind)) return MATTEN_EINVAL;
    if (!g || !count) return MATTEN_EINVAL;
    if (n_rows == 0) return MATTEN_OK;
    if (!pred || !target || !selector || !grad_pred) return MATTEN_EINVAL;
    const int64_t n = n_rows * d;
    const unsigned blocks = (unsigned)matten_cdiv(n, SL_THREADS);
    if (kind == 0)
        selected_bwd_kernel<0><<<blocks, SL_THREADS, 0, stream>>>(pred, target, selector, (uint32_t)n, (uint32_t)d, g, count,
                                                                  grad_pred);
    else
        selected_bwd_kernel<1><<<blocks, SL_THREADS, 0, stream>>>(pred, target, selector, (uint32_t)n, (uint32_t)d, g, count,
                                                                  grad_pred);
    MATTEN_LAUNCH_CHECK();
    return MATTEN_OK;
}
