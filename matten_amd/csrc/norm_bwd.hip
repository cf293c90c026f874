// Adjoints of the activation followed by eval-mode BatchNorm (frozen running statistics):
//   y = BN_eval(Gate(x))            reference nn/utils.py:96-141 (Gate) + 414-418 (BatchNorm, not training)
//   y = BN_eval(NormActivation(x))  reference nn/utils.py:142-150 + 414-418
// With running statistics the BatchNorm is a per-channel affine map of the activated value a:
//   0e channels: (a - running_mean) rsqrt(running_var + eps) weight + bias,   others: a rsqrt(running_var + eps) weight
// so  da = dy * scale,  dweight[c] = rsqrt(var + eps) sum dy (a - mean),  dbias = sum dy  (sums over rows and components).
// The forward is matten_gate_bn / matten_norm_act with the running statistics; nothing but x is kept for the adjoint, the
// activated value is re-evaluated here.  One pass over x and dy gives dx and, per (EB_ROWS-row block, column), a partial
// record (sum dy (a - mean), sum dy); a second launch adds a channel's records in a fixed order: no atomics, bitwise
// reproducible, the running statistics are only read.
#include "common.h"

namespace {

__device__ __forceinline__ float sigmoidf_(float v) { return 1.0f / (1.0f + expf(-v)); }
__device__ __forceinline__ float act_f(int code, float v) {   // as backward.hip
    switch (code) {
        case 1: return v * sigmoidf_(v);
        case 2: return tanhf(v);
        case 3: return sigmoidf_(v);
        case 4: return (v > 20.0f ? v : log1pf(expf(v))) - 0.6931471805599453f;
        case 5: return fabsf(v);
        default: return v;
    }
}
__device__ __forceinline__ float act_df(int code, float v) {
    switch (code) {
        case 1: { float s = sigmoidf_(v); return s * (1.0f + v * (1.0f - s)); }
        case 2: { float t = tanhf(v); return 1.0f - t * t; }
        case 3: { float s = sigmoidf_(v); return s * (1.0f - s); }
        case 4: return sigmoidf_(v);
        case 5: return v > 0.0f ? 1.0f : (v < 0.0f ? -1.0f : 0.0f);
        default: return 1.0f;
    }
}

constexpr int EB_ROWS = 16;    // rows per workgroup = rows per partial record
constexpr int EB_UNROLL = 8;   // rows whose loads are in flight together (as gate_bn_kernel)

// Gate.  The layout of gate_bn_kernel: a thread owns OUTPUT column o (its source / gate column, activation codes and the
// folded BatchNorm scale in registers) and walks the workgroup's rows, consecutive threads consecutive columns.  It writes
// dx of its source column; the thread of a gated channel's first component also writes the gate's dx, the channel's 2l+1
// terms summed in component order (their x and dy were just read by the neighbouring lanes: cache hits).
// meta[d_out] int4 {src, gate (-1: scalar), act | gate_act << 8, bn channel | mean index << 16 (0xffff: not centred)}
template <bool PARAM_GRADS>
__global__ __launch_bounds__(256) void gate_bn_eval_bwd_kernel(const float* __restrict__ x, int d_in,
                                                               const int4* __restrict__ meta, int d_out,
                                                               const float* __restrict__ act_cst,
                                                               const float* __restrict__ running_mean,
                                                               const float* __restrict__ running_var,
                                                               const float* __restrict__ bn_weight, float eps,
                                                               const float* __restrict__ dy, int64_t n_rows,
                                                               float* __restrict__ dx, float2* __restrict__ part) {
    const int o = blockIdx.y * blockDim.x + threadIdx.x;
    if (o >= d_out) return;
    const int4 m = meta[o];
    const int act = m.z & 0xff, gact = (m.z >> 8) & 0xff;
    const float ca = act ? act_cst[act] : 1.0f, cg = gact ? act_cst[gact] : 1.0f;
    const int bn_idx = m.w & 0xffff, mean_idx = (m.w >> 16) & 0xffff;
    const float scale = bn_weight[bn_idx] / sqrtf(running_var[bn_idx] + eps);   // the forward's folding
    const float mu = mean_idx != 0xffff ? running_mean[mean_idx] : 0.0f;
    const bool gated = m.y >= 0;
    const int gcol = gated ? m.y : m.x;   // scalars read their own column twice (no branch around a load)
    int nk = 0;                           // components of the channel, on the thread of its first one
    if (gated && (o == 0 || meta[o - 1].y != m.y)) {
        nk = 1;
        while (o + nk < d_out && meta[o + nk].y == m.y) ++nk;
    }
    const int64_t row0 = (int64_t)blockIdx.x * EB_ROWS;
    const int rows = (int)min((int64_t)EB_ROWS, n_rows - row0);
    float A = 0.0f, B = 0.0f;
    for (int r0 = 0; r0 < rows; r0 += EB_UNROLL) {
        float a[EB_UNROLL], b[EB_UNROLL], g[EB_UNROLL];
#pragma unroll
        for (int i = 0; i < EB_UNROLL; ++i) {
            const int64_t r = row0 + min(r0 + i, rows - 1);
            a[i] = x[r * d_in + m.x];
            b[i] = x[r * d_in + gcol];
            g[i] = dy[r * d_out + o];
        }
#pragma unroll
        for (int i = 0; i < EB_UNROLL; ++i) {
            if (r0 + i < rows) {
                const int64_t r = row0 + r0 + i;
                const float v = a[i], gs = g[i] * scale;   // dL/d(activated value)
                float av;
                if (!gated) {
                    av = act ? act_f(act, v) * ca : v;
                    dx[r * d_in + m.x] = act ? gs * act_df(act, v) * ca : gs;
                } else {
                    const float gte = gact ? act_f(gact, b[i]) * cg : b[i];
                    av = v * gte;
                    dx[r * d_in + m.x] = gs * gte;
                    if (nk) {
                        float sum = 0.0f;
                        for (int kk = 0; kk < nk; ++kk)
                            sum = fmaf(dy[r * d_out + o + kk], x[r * d_in + meta[o + kk].x], sum);
                        dx[r * d_in + m.y] = sum * scale * (gact ? act_df(gact, b[i]) * cg : 1.0f);
                    }
                }
                if (PARAM_GRADS) {
                    A = fmaf(g[i], av - mu, A);
                    B += g[i];
                }
            }
        }
    }
    if (PARAM_GRADS) part[(int64_t)blockIdx.x * d_out + o] = make_float2(A, B);
}

// NormActivation.  A thread owns CHANNEL c (its 2l+1 columns are contiguous: neighbouring lanes read neighbouring
// pieces of the row) and walks the workgroup's rows; records are per (row block, channel).
// chan[C] int4 {offset, d, is_0e, mean index} (plan_batchnorm)
template <bool PARAM_GRADS>
__global__ __launch_bounds__(256) void norm_act_bn_eval_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                                   int dim, int64_t n_rows, const int4* __restrict__ chan,
                                                                   int n_chan, int act, float eps2,
                                                                   const float* __restrict__ running_mean,
                                                                   const float* __restrict__ running_var,
                                                                   const float* __restrict__ bn_weight, float bn_eps,
                                                                   float* __restrict__ dx, float2* __restrict__ part) {
    const int c = blockIdx.y * blockDim.x + threadIdx.x;
    if (c >= n_chan) return;
    const int4 ch = chan[c];
    const float bs = bn_weight[c] / sqrtf(running_var[c] + bn_eps);
    const float mu = ch.z ? running_mean[ch.w] : 0.0f;
    const int64_t row0 = (int64_t)blockIdx.x * EB_ROWS;
    const int rows = (int)min((int64_t)EB_ROWS, n_rows - row0);
    float A = 0.0f, B = 0.0f;
    for (int r = 0; r < rows; ++r) {
        const float* xp = x + (row0 + r) * dim + ch.x;
        const float* gp = dy + (row0 + r) * dim + ch.x;
        float* dp = dx + (row0 + r) * dim + ch.x;
        float n2 = 0.0f, gx = 0.0f;
        for (int k = 0; k < ch.y; ++k) {
            n2 = fmaf(xp[k], xp[k], n2);
            gx = fmaf(gp[k], xp[k], gx);
        }
        const float nn = sqrtf(fmaxf(n2, eps2));
        const float f = act_f(act, nn), s = f / nn;
        // (a clamped norm is a constant, as in norm_act_bwd_kernel)
        const float t = n2 < eps2 ? 0.0f : (act_df(act, nn) * nn - f) / (nn * nn * nn) * (gx * bs);
        const float sb = s * bs;
        for (int k = 0; k < ch.y; ++k) {
            const float xv = xp[k], g = gp[k];
            dp[k] = fmaf(t, xv, sb * g);
            if (PARAM_GRADS) {
                A = fmaf(g, fmaf(s, xv, -mu), A);
                B += g;
            }
        }
    }
    if (PARAM_GRADS) part[(int64_t)blockIdx.x * n_chan + c] = make_float2(A, B);
}

// second stage: channel c = one workgroup; thread t adds records t, t + 256, ... in order, then a fixed tree.
// Records per column (ld = row width, a channel's d columns at chan[c].x) or per channel (per_channel: ld = n_chan).
__global__ __launch_bounds__(256) void bn_eval_bwd_finish_kernel(const float2* __restrict__ part, int ld, int64_t n_blocks,
                                                                 const int4* __restrict__ chan, int per_channel,
                                                                 const float* __restrict__ running_var, float eps,
                                                                 float* __restrict__ dweight, float* __restrict__ dbias) {
    __shared__ float ra[256], rb[256];
    const int c = blockIdx.x, t = threadIdx.x;
    const int4 ch = chan[c];
    const int off = per_channel ? c : ch.x, d = per_channel ? 1 : ch.y;
    float a = 0.0f, b = 0.0f;
    const int64_t items = n_blocks * d;
    for (int64_t i = t; i < items; i += 256) {
        const float2 p = part[(i / d) * ld + off + (int)(i % d)];
        a += p.x;
        b += p.y;
    }
    ra[t] = a, rb[t] = b;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) ra[t] += ra[t + o], rb[t] += rb[t + o];
        __syncthreads();
    }
    if (t == 0) {
        dweight[c] = ra[0] / sqrtf(running_var[c] + eps);
        if (ch.z && dbias) dbias[ch.w] = rb[0];
    }
}

}  // namespace

extern "C" int64_t matten_bn_eval_bwd_scratch_floats(int64_t n_rows, int64_t n_cols) {
    return n_rows > 0 && n_cols > 0 ? 2 * matten_cdiv(n_rows, EB_ROWS) * n_cols : 0;
}

extern "C" int matten_gate_bn_eval_bwd(const float* x, int64_t d_in, const int32_t* meta, int64_t d_out, const float* act_cst,
                                       const int32_t* bn_chan, int64_t n_chan, const float* running_mean,
                                       const float* running_var, const float* bn_weight, float eps, const float* dy,
                                       int64_t n_rows, float* dx, float* dweight, float* dbias, float* scratch,
                                       matten_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (n_rows <= 0 || d_in <= 0 || d_out <= 0 || n_chan <= 0) return MATTEN_EINVAL;
    if (!x || !meta || !act_cst || !running_var || !bn_weight || !dy || !dx) return MATTEN_EINVAL;
    if (dweight && (!scratch || !bn_chan)) return MATTEN_EINVAL;
    const int64_t n_blocks = matten_cdiv(n_rows, EB_ROWS);
    if (n_blocks >= ((int64_t)1 << 31)) return MATTEN_EINVAL;
    const int TC = (int)(d_out >= 256 ? 256 : 64 * matten_cdiv(d_out, 64));   // whole waves, at most one of them part idle
    dim3 grid((unsigned)n_blocks, (unsigned)matten_cdiv(d_out, TC));
    if (dweight) {
        gate_bn_eval_bwd_kernel<true><<<grid, TC, 0, stream>>>(x, (int)d_in, (const int4*)meta, (int)d_out, act_cst,
                                                               running_mean, running_var, bn_weight, eps, dy, n_rows, dx,
                                                               (float2*)scratch);
        MATTEN_LAUNCH_CHECK();
        bn_eval_bwd_finish_kernel<<<(unsigned)n_chan, 256, 0, stream>>>((const float2*)scratch, (int)d_out, n_blocks,
                                                                        (const int4*)bn_chan, 0, running_var, eps, dweight,
                                                                        dbias);
    } else {
        gate_bn_eval_bwd_kernel<false><<<grid, TC, 0, stream>>>(x, (int)d_in, (const int4*)meta, (int)d_out, act_cst,
                                                                running_mean, running_var, bn_weight, eps, dy, n_rows, dx,
                                                                nullptr);
    }
    MATTEN_LAUNCH_CHECK();
    return MATTEN_OK;
}

extern "C" int matten_norm_act_bn_eval_bwd(const float* x, const float* dy, int64_t dim, int64_t n_rows, const int32_t* chan,
                                           int64_t n_chan, int act, float epsilon, const float* running_mean,
                                           const float* running_var, const float* bn_weight, float bn_eps, float* dx,
                                           float* dweight, float* dbias, float* scratch, matten_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (n_rows <= 0 || dim <= 0 || n_chan <= 0 || act < 1 || act > 5 || !(epsilon > 0.0f)) return MATTEN_EINVAL;
    if (!x || !dy || !chan || !running_var || !bn_weight || !dx) return MATTEN_EINVAL;
    if (dweight && !scratch) return MATTEN_EINVAL;
    const int64_t n_blocks = matten_cdiv(n_rows, EB_ROWS);
    if (n_blocks >= ((int64_t)1 << 31)) return MATTEN_EINVAL;
    const int TC = (int)(n_chan >= 256 ? 256 : 64 * matten_cdiv(n_chan, 64));
    dim3 grid((unsigned)n_blocks, (unsigned)matten_cdiv(n_chan, TC));
    if (dweight) {
        norm_act_bn_eval_bwd_kernel<true><<<grid, TC, 0, stream>>>(x, dy, (int)dim, n_rows, (const int4*)chan, (int)n_chan, act,
                                                                   epsilon * epsilon, running_mean, running_var, bn_weight,
                                                                   bn_eps, dx, (float2*)scratch);
        MATTEN_LAUNCH_CHECK();
        bn_eval_bwd_finish_kernel<<<(unsigned)n_chan, 256, 0, stream>>>((const float2*)scratch, (int)n_chan, n_blocks,
                                                                        (const int4*)chan, 1, running_var, bn_eps, dweight,
                                                                        dbias);
    } else {
        norm_act_bn_eval_bwd_kernel<false><<<grid, TC, 0, stream>>>(x, dy, (int)dim, n_rows, (const int4*)chan, (int)n_chan, act,
                                                                    epsilon * epsilon, running_mean, running_var, bn_weight,
                                                                    bn_eps, dx, nullptr);
    }
    MATTEN_LAUNCH_CHECK();
    return MATTEN_OK;
}
