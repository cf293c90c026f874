// Adam over ONE flat fp32 parameter buffer (the reference configures torch.optim.Adam,
// scripts/configs/materials_tensor.yaml:103-107: lr 0.01, weight_decay 1e-5 = L2 term added to the gradient).
//
// The model's ~60 parameter tensors are views into one buffer (matten_amd/optim.py), so are their gradients: a step is
// one elementwise launch over 3.5 M floats (56 MB of traffic: p, g read, m, v read and written, p written), and
// zeroing the gradients one memset.  The step count lives on the device (hipGraph capture: nothing on the host changes
// between replays); the bias corrections are computed per thread from it.
//   g' = g + wd p;  m = b1 m + (1 - b1) g';  v = b2 v + (1 - b2) g'^2
//   p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)          (torch.optim.Adam, amsgrad = False)
#include "common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                   float* __restrict__ v, int64_t n, const float* __restrict__ step, float lr,
                                                   float b1, float b2, float eps, float wd) {
    const float t = step[0];                       // already incremented by the caller for this step
    const float c1 = 1.0f - powf(b1, t), c2s = sqrtf(1.0f - powf(b2, t));
    const float step_size = lr / c1;
    const int64_t i4 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i4 >= n) return;
    if (i4 + 4 <= n) {
        f32x4 pp = *reinterpret_cast<f32x4*>(p + i4), mm = *reinterpret_cast<f32x4*>(m + i4),
              vv = *reinterpret_cast<f32x4*>(v + i4);
        const f32x4 gg = *reinterpret_cast<const f32x4*>(g + i4);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float gk = gg[k] + wd * pp[k];
            mm[k] = b1 * mm[k] + (1.0f - b1) * gk;
            vv[k] = b2 * vv[k] + (1.0f - b2) * gk * gk;
            pp[k] -= step_size * mm[k] / (sqrtf(vv[k]) / c2s + eps);
        }
        *reinterpret_cast<f32x4*>(p + i4) = pp;
        *reinterpret_cast<f32x4*>(m + i4) = mm;
        *reinterpret_cast<f32x4*>(v + i4) = vv;
    } else {
        for (int64_t i = i4; i < n; ++i) {
            const float gk = g[i] + wd * p[i];
            m[i] = b1 * m[i] + (1.0f - b1) * gk;
            v[i] = b2 * v[i] + (1.0f - b2) * gk * gk;
            p[i] -= step_size * m[i] / (sqrtf(v[i]) / c2s + eps);
        }
    }
}


// ---------------------------------------------------------------------------------------------------------------------
// The step with its controls on the device (matten_adam_step_ctl): global-norm clipping, a guard against non-finite
// gradients, decoupled weight decay, an EMA of the parameters and a learning rate read from device memory -- a chain
// of at most three launches on ONE stream with nothing read back, so it captures into a hipGraph as it is and a replay
// follows whatever the host last wrote into ctl[0].
//   A  sumsq_kernel      one fp64 partial per workgroup of sum g^2            (only with clipping or the guard)
//   B  control_kernel    one workgroup: norm, scale, skip; advances the step count unless the step is skipped
//   C  adam_ctl_kernel   the update, every thread reading lr / scale / skip / step from what B left
// The number of workgroups of A is a function of n alone and every sum runs in a fixed order (lane: ascending index;
// wave: xor butterfly; workgroup and the partials: ascending), so the norm -- and with it the whole step -- has the same
// bits on every device and in every run.  No floating-point atomics.
constexpr int SUMSQ_THREADS = 256;
constexpr int SUMSQ_TILE = SUMSQ_THREADS * 4;     // floats one workgroup takes per round of 16-byte loads
constexpr int SUMSQ_MAX_BLOCKS = 1024;            // 3.5 M floats: 1024 workgroups, four loads in flight per lane

__host__ __device__ inline int64_t sumsq_blocks(int64_t n) {
    const int64_t b = (n + SUMSQ_TILE - 1) / SUMSQ_TILE;
    return b < 1 ? 1 : (b > SUMSQ_MAX_BLOCKS ? SUMSQ_MAX_BLOCKS : b);
}

// sum over the workgroup, valid in thread 0: butterfly inside each 64-wide wave, then the waves in index order
template <int THREADS>
__device__ inline double block_sum_ordered(double x, double* lds) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) x += __shfl_xor(x, off, 64);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) lds[wave] = x;
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x == 0)
        for (int w = 0; w < THREADS / 64; ++w) s += lds[w];
    return s;
}

__global__ __launch_bounds__(SUMSQ_THREADS) void sumsq_kernel(const float* __restrict__ g, int64_t n,
                                                              double* __restrict__ partials) {
    __shared__ double lds[SUMSQ_THREADS / 64];
    const int64_t nv = n >> 2;                                                  // whole 16-byte vectors
    const int64_t stride = (int64_t)gridDim.x * SUMSQ_THREADS;
    const f32x4* __restrict__ g4 = reinterpret_cast<const f32x4*>(g);
    double acc = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * SUMSQ_THREADS + threadIdx.x; i < nv; i += 4 * stride) {
        f32x4 x[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {                                           // four independent loads before the first use
            const int64_t j = i + u * stride;
            x[u] = j < nv ? g4[j] : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int k = 0; k < 4; ++k) acc = fma((double)x[u][k], (double)x[u][k], acc);   // fp32 squares are exact in fp64
    }
    if (blockIdx.x == 0 && (int64_t)threadIdx.x < n - 4 * nv) {                 // up to three floats behind the last vector
        const double t = (double)g[4 * nv + threadIdx.x];
        acc = fma(t, t, acc);
    }
    const double s = block_sum_ordered<SUMSQ_THREADS>(acc, lds);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// ctl[0] lr (in), [1] norm, [2] scale; counters[0] skipped steps so far, [1] this step skipped; step[0] += !skip
__global__ __launch_bounds__(256) void control_kernel(const double* __restrict__ partials, int n_partials, float max_norm,
                                                      int guard, float* __restrict__ ctl, int32_t* __restrict__ counters,
                                                      float* __restrict__ step) {
    __shared__ double lds[4];
    double acc = 0.0;
    for (int j = threadIdx.x; j < n_partials; j += 256) acc += partials[j];
    const double sum = block_sum_ordered<256>(acc, lds);
    if (threadIdx.x != 0) return;
    float norm = __builtin_nanf(""), scale = 1.0f;
    int skip = 0;
    if (n_partials > 0) {
        norm = (float)sqrt(sum);
        if (max_norm > 0.0f) {
            const float s = max_norm / (norm + 1e-6f);      // torch.nn.utils.clip_grad_norm_
            scale = s > 1.0f ? 1.0f : s;                    // a NaN norm stays a NaN scale (clamp(max=1), not fminf)
        }
        skip = guard && !isfinite(sum);
    }
    ctl[1] = norm;
    ctl[2] = scale;
    counters[0] += skip;
    counters[1] = skip;
    step[0] += skip ? 0.0f : 1.0f;
}

template <bool DECOUPLED, bool EMA>
__device__ inline void adam_ctl_update(float& p, float g, float& m, float& v, float& e, float step_size, float c2s, float lr,
                                       float scale, float b1, float b2, float eps, float wd, float d) {
    float gk = scale * g;
    if (DECOUPLED) p *= 1.0f - lr * wd;                     // torch.optim.AdamW
    else gk += wd * p;
    m = b1 * m + (1.0f - b1) * gk;
    v = b2 * v + (1.0f - b2) * gk * gk;
    p -= step_size * m / (sqrtf(v) / c2s + eps);
    if (EMA) e = d * e + (1.0f - d) * p;
}

template <bool DECOUPLED, bool EMA>
__global__ __launch_bounds__(256) void adam_ctl_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                       float* __restrict__ m, float* __restrict__ v,
                                                       float* __restrict__ ema, int64_t n, const float* __restrict__ step,
                                                       const float* __restrict__ ctl, const int32_t* __restrict__ counters,
                                                       float b1, float b2, float eps, float wd, float d) {
    if (counters[1]) return;                                // skipped: p, m, v, ema keep their bits
    const float t = step[0], lr = ctl[0], scale = ctl[2];   // written before this launch, read-only here
    const float c1 = 1.0f - powf(b1, t), c2s = sqrtf(1.0f - powf(b2, t));
    const float step_size = lr / c1;
    const int64_t i4 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i4 >= n) return;
    if (i4 + 4 <= n) {
        f32x4 pp = *reinterpret_cast<f32x4*>(p + i4), mm = *reinterpret_cast<f32x4*>(m + i4),
              vv = *reinterpret_cast<f32x4*>(v + i4), ee = {0.0f, 0.0f, 0.0f, 0.0f};
        const f32x4 gg = *reinterpret_cast<const f32x4*>(g + i4);
        if (EMA) ee = *reinterpret_cast<f32x4*>(ema + i4);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float pk = pp[k], mk = mm[k], vk = vv[k], ek = ee[k];
            adam_ctl_update<DECOUPLED, EMA>(pk, gg[k], mk, vk, ek, step_size, c2s, lr, scale, b1, b2, eps, wd, d);
            pp[k] = pk, mm[k] = mk, vv[k] = vk, ee[k] = ek;
        }
        *reinterpret_cast<f32x4*>(p + i4) = pp;
        *reinterpret_cast<f32x4*>(m + i4) = mm;
        *reinterpret_cast<f32x4*>(v + i4) = vv;
        if (EMA) *reinterpret_cast<f32x4*>(ema + i4) = ee;
    } else {
        for (int64_t i = i4; i < n; ++i) {
            float ek = EMA ? ema[i] : 0.0f;
            adam_ctl_update<DECOUPLED, EMA>(p[i], g[i], m[i], v[i], ek, step_size, c2s, lr, scale, b1, b2, eps, wd, d);
            if (EMA) ema[i] = ek;
        }
    }
}

}  // namespace

extern "C" int matten_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n,
                                const float* step, float lr, float beta1, float beta2, float eps, float weight_decay,
                                matten_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (n < 0 || !(lr >= 0.0f) || !(beta1 >= 0.0f && beta1 < 1.0f) || !(beta2 >= 0.0f && beta2 < 1.0f) || !(eps >= 0.0f))
        return MATTEN_EINVAL;
    if (n == 0) return MATTEN_OK;
    if (!params || !grads || !exp_avg || !exp_avg_sq || !step) return MATTEN_EINVAL;
    if ((reinterpret_cast<uintptr_t>(params) | reinterpret_cast<uintptr_t>(grads) | reinterpret_cast<uintptr_t>(exp_avg) |
         reinterpret_cast<uintptr_t>(exp_avg_sq)) & 15)
        return MATTEN_EINVAL;
    const int64_t blocks = matten_cdiv(matten_cdiv(n, 4), 256);
    if (blocks >= ((int64_t)1 << 31)) return MATTEN_EINVAL;
    adam_kernel<<<(unsigned)blocks, 256, 0, stream>>>(params, grads, exp_avg, exp_avg_sq, n, step, lr, beta1, beta2, eps,
                                                      weight_decay);
    MATTEN_LAUNCH_CHECK();
    return MATTEN_OK;
}

extern "C" size_t matten_adam_ctl_workspace_bytes(int64_t n) {
    return n > 0 ? (size_t)sumsq_blocks(n) * sizeof(double) : 0;
}

extern "C" int matten_adam_step_ctl(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* ema,
                                    int64_t n, float* step, float* ctl, int32_t* counters, void* workspace,
                                    size_t workspace_bytes, float max_norm, float beta1, float beta2, float eps,
                                    float weight_decay, float ema_decay, int decoupled, int guard, matten_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (n < 0 || !(beta1 >= 0.0f && beta1 < 1.0f) || !(beta2 >= 0.0f && beta2 < 1.0f) || !(eps >= 0.0f) ||
        !(ema_decay >= 0.0f && ema_decay < 1.0f) || !(max_norm >= 0.0f))
        return MATTEN_EINVAL;
    if (n == 0) return MATTEN_OK;
    if (!params || !grads || !exp_avg || !exp_avg_sq || !step || !ctl || !counters || !workspace) return MATTEN_EINVAL;
    if ((reinterpret_cast<uintptr_t>(params) | reinterpret_cast<uintptr_t>(grads) | reinterpret_cast<uintptr_t>(exp_avg) |
         reinterpret_cast<uintptr_t>(exp_avg_sq) | reinterpret_cast<uintptr_t>(ema)) & 15)
        return MATTEN_EINVAL;
    if (reinterpret_cast<uintptr_t>(workspace) & 7) return MATTEN_EINVAL;
    if (workspace_bytes < matten_adam_ctl_workspace_bytes(n)) return MATTEN_EINVAL;
    const int64_t blocks = matten_cdiv(matten_cdiv(n, 4), 256);
    if (blocks >= ((int64_t)1 << 31)) return MATTEN_EINVAL;
    double* partials = static_cast<double*>(workspace);
    int n_partials = 0;
    if (max_norm > 0.0f || guard) {
        n_partials = (int)sumsq_blocks(n);
        sumsq_kernel<<<(unsigned)n_partials, SUMSQ_THREADS, 0, stream>>>(grads, n, partials);
        MATTEN_LAUNCH_CHECK();
    }
    control_kernel<<<1, 256, 0, stream>>>(partials, n_partials, max_norm, guard ? 1 : 0, ctl, counters, step);
    MATTEN_LAUNCH_CHECK();
#define MATTEN_ADAM_CTL(DEC, EMA)                                                                                          \
    adam_ctl_kernel<DEC, EMA><<<(unsigned)blocks, 256, 0, stream>>>(params, grads, exp_avg, exp_avg_sq, ema, n, step, ctl, \
                                                                    counters, beta1, beta2, eps, weight_decay, ema_decay)
    if (decoupled) {
        if (ema) MATTEN_ADAM_CTL(true, true);
        else MATTEN_ADAM_CTL(true, false);
    } else {
        if (ema) MATTEN_ADAM_CTL(false, true);
        else MATTEN_ADAM_CTL(false, false);
    }
#undef MATTEN_ADAM_CTL
    MATTEN_LAUNCH_CHECK();
    return MATTEN_OK;
}
