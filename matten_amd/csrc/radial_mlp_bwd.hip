// Adjoint of the radial MLP (training step): given dL/dw[E, w_ld] from the tensor-product adjoint, the gradients of the
// bias-free layers of e3nn FullyConnectedNet([nb] + L x [32] + [W], silu)  (reference nn/utils.py:246-251,260; the
// reference gets them from autograd through torch.mm).  The comments below spell out the shipped L = 2 (N_MID = 1
// middle layer W1p); every kernel takes N_MID = L - 1 in 0..3 as a template parameter and chains all middle layers the
// same way (z_{i+1} = h_i Wm_i, dh_i = dz_{i+1} Wm_i^T, dWm_i = h_i^T dz_{i+1}).
//
// In the packed form the forward kernel (radial_mlp.hip) evaluates:
//      b = bessel(|v|) [nb]   z1 = b W0p   h1 = silu(z1)   z2 = h1 W1p   h2 = silu(z2)   w = h2 W2p
// (the 1/sqrt(fan_in) and normalize2mom factors live in W0p, W1p, W2p; the host maps the packed gradients back).
//      dh2 = dw W2p^T          dW2p = h2^T dw
//      dz2 = dh2 * silu'(z2)   dW1p = h1^T dz2     dh1 = dz2 W1p^T
//      dz1 = dh1 * silu'(z1)   dW0p = b^T dz1
// Layers of 128 to 512 weight columns run ONE kernel that reads dw once (radial_mlp_bwd_fused below); narrower / wider
// ones two kernels, both on the fp32 matrix cores (v_mfma_f32_16x16x4_f32), both reading dw once:
//   radial_mlp_bwd_edges   a wave owns tiles of 16 edges (edges = the N dimension, like the forward kernel): recomputes
//                          z1, h1, z2, h2 in registers, contracts dw with W2p over the weight columns (16 bytes per lane
//                          and row: whole 64-byte pieces of 16 rows per load, the four floats being the B operands of
//                          four matrix steps), chains dz2 -> dh1 -> dz1 in registers (the D fragment of one layer is the B
//                          operand of the next, as in the forward kernel), writes h2 for the second kernel, and sums the
//                          two small weight gradients over its edges (operands transposed through a wave-private LDS
//                          tile: there the contraction runs over the edges)
//   radial_mlp_bwd_w2      dW2p[k, q] = sum_e h2[e, k] dw[e, q]: a wave owns 16 weight columns and an edge range
// Both write PARTIAL sums (one slice per wave / per edge range) that the host adds up in a fixed order: no atomics,
// bit-reproducible.  dw may be fp32 or bf16 (the opt-in bf16 storage of the per-edge tensors).
#include <algorithm>

#include <hip/hip_bf16.h>

#include "common.h"
#include "sh.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int HID = 32;
constexpr int BW_WAVES = 4;
#ifndef BW_WAVES_TARGET
#define BW_WAVES_TARGET 2048   // waves' worth of tiles before a wave takes more than one
#endif
#ifndef BW_TILES_MAX_N
#define BW_TILES_MAX_N 8
#endif
constexpr int BW_TILES_MAX = BW_TILES_MAX_N;      // 16-edge tiles per wave of radial_mlp_bwd_edges: fewer on small graphs (see bw_tiles)
constexpr int TS = 17;               // row stride of the LDS transpose tiles (16 edges + 1: bank spread)
constexpr int W2_RANGE_MAX = 4096;   // edges per partial sum of radial_mlp_bwd_w2: fewer on small graphs (see w2_range)

// Small graphs (a training batch of 32 crystals has ~4 k edges) need the parallelism more than the short partial lists:
// a wave takes one tile / a range is 256 edges until there are ~2000 waves' worth of work.
inline int bw_tiles(int64_t n_edges) {
    const int64_t t = n_edges / (16 * BW_WAVES_TARGET);
    return (int)(t < 1 ? 1 : (t > BW_TILES_MAX ? BW_TILES_MAX : t));
}
// enough (column group, edge range) workgroups to fill the chip (~1024): a launch with 48 weight columns has ONE column
// group, and 72 ranges of 4096 edges each left 184 CUs idle while three waves per workgroup walked 256 dependent steps
// (0.31 ms for the first conv layer's 48 columns at 293 k edges; LAB_NOTES round 4)
inline int w2_range(int64_t n_edges, int64_t w_pad) {
    const int64_t groups = (w_pad + 16 * BW_WAVES - 1) / (16 * BW_WAVES);
    int64_t r = (n_edges * groups / 1024 + 15) / 16 * 16;
    return (int)(r < 256 ? 256 : (r > W2_RANGE_MAX ? W2_RANGE_MAX : r));
}

__device__ __forceinline__ float silu(float z) { return z / (1.0f + expf(-z)); }
__device__ __forceinline__ float dsilu(float z) {
    const float s = 1.0f / (1.0f + expf(-z));
    return s * (1.0f + z * (1.0f - s));
}

template <bool BF16>
__device__ __forceinline__ f32x4 load4(const void* base, int64_t idx) {   // 4 consecutive elements at element index idx
    if constexpr (BF16) {
        const uint2 raw = *reinterpret_cast<const uint2*>(reinterpret_cast<const uint16_t*>(base) + idx);
        return f32x4{__uint_as_float(raw.x << 16), __uint_as_float(raw.x & 0xffff0000u), __uint_as_float(raw.y << 16),
                     __uint_as_float(raw.y & 0xffff0000u)};
    } else {
        return *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(base) + idx);
    }
}
template <bool BF16>
__device__ __forceinline__ float load1(const void* base, int64_t idx) {
    if constexpr (BF16) return __uint_as_float((uint32_t)reinterpret_cast<const uint16_t*>(base)[idx] << 16);
    else return reinterpret_cast<const float*>(base)[idx];
}

// middle-layer arrays keep one element at N_MID = 0 (unused)
constexpr int nm1(int n) { return n > 0 ? n : 1; }

// The small weight gradients of one 16-edge tile: contraction over the tile's edges, operands transposed through the
// wave's LDS tiles (t_h1 / t_dz2: input and output-gradient of a middle layer, t_dz1 / t_b: those of layer 0).  Pass p
// adds dWm_p += h_p^T dz_{p+1}; pass 0 adds dW0 += b^T dz_0 too.  Passes N_MID-1 .. 0, one tile write + read each.
template <int KS0, int N_MID>
__device__ __forceinline__ void small_grads_tile(float* t_h1, float* t_dz2, float* t_dz1, float* t_b, const f32x4 (&h)[nm1(N_MID)][2],
                                                 const f32x4 (&dz)[N_MID + 1][2], const float (&bes)[KS0], int g, int c,
                                                 f32x4 (&g_wm)[nm1(N_MID)][2][2], f32x4 (&g_w0)[2]) {
#pragma unroll
    for (int p = (N_MID > 0 ? N_MID - 1 : 0); p >= 0; --p) {
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int k = 16 * t + 4 * g + r;
                if (p < N_MID) {
                    t_h1[k * TS + c] = h[p][t][r];
                    t_dz2[k * TS + c] = dz[p < N_MID ? p + 1 : 0][t][r];
                }
                if (p == 0) t_dz1[k * TS + c] = dz[0][t][r];
            }
        if (p == 0) {
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) t_b[(4 * kk + g) * TS + c] = kk < KS0 ? bes[kk < KS0 ? kk : 0] : 0.0f;
        }
        __builtin_amdgcn_s_waitcnt(0xc07f);
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int s = 0; s < 4; ++s) {   // K step s: edges 4 s + g
            const int ee = 4 * s + g;
            if (p < N_MID) {
                const float h1a = t_h1[c * TS + ee], h1b = t_h1[(16 + c) * TS + ee];
                const float d2a = t_dz2[c * TS + ee], d2b = t_dz2[(16 + c) * TS + ee];
                f32x4 (&gw)[2][2] = g_wm[p < N_MID ? p : 0];
                gw[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(h1a, d2a, gw[0][0], 0, 0, 0);
                gw[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(h1a, d2b, gw[0][1], 0, 0, 0);
                gw[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(h1b, d2a, gw[1][0], 0, 0, 0);
                gw[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(h1b, d2b, gw[1][1], 0, 0, 0);
            }
            if (p == 0) {
                const float d1a = t_dz1[c * TS + ee], d1b = t_dz1[(16 + c) * TS + ee];
                const float bb = t_b[c * TS + ee];
                g_w0[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(bb, d1a, g_w0[0], 0, 0, 0);
                g_w0[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(bb, d1b, g_w0[1], 0, 0, 0);
            }
        }
        if (p > 0) __builtin_amdgcn_wave_barrier();   // (pass 0: the caller's barrier follows)
    }
}

// this wave's partial sums of the small gradients: D[row 4 g + r][col c]; slice = [nb_pad*32 (dW0p) + N_MID*32*32 (dWm_p)]
template <int KS0, int N_MID>
__device__ __forceinline__ void store_small(float* out, const f32x4 (&g_w0)[2], const f32x4 (&g_wm)[nm1(N_MID)][2][2], int g,
                                            int c, float s0, float s1) {
    const int nb_pad = 4 * KS0;
#pragma unroll
    for (int tn = 0; tn < 2; ++tn)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int k0 = 4 * g + r;
            if (k0 < nb_pad) out[k0 * HID + 16 * tn + c] = g_w0[tn][r] * s0;
        }
#pragma unroll
    for (int m = 0; m < N_MID; ++m) {
        float* out1 = out + nb_pad * HID + m * HID * HID;
#pragma unroll
        for (int tm = 0; tm < 2; ++tm)
#pragma unroll
            for (int tn = 0; tn < 2; ++tn)
#pragma unroll
                for (int r = 0; r < 4; ++r) out1[(16 * tm + 4 * g + r) * HID + 16 * tn + c] = g_wm[m][tm][tn][r] * s1;
    }
}

// d/dr of matten::bessel_basis (sh.h): b_k = A sin(a x) / x, a = (k+1) pi / c  ->  b_k' = A a^2 (t cos t - sin t) / t^2, t = a x
// (below t = 0.5 the difference cancels: its series -t/3 + t^3/30 - t^5/840 + t^7/45360, next term < 5e-10); 0 where b_k is
__device__ __forceinline__ float bessel_basis_dr(float len, int k, int n_basis, float r_start, float r_end) {
    const float xr = len - r_start;
    const float c = r_end - r_start;
    const bool in = (xr / c < 1.0f) && (0.0f < xr);
    const float a = (float)(k + 1) * 3.14159265358979323846f / c;
    const float t = (float)(k + 1) * 3.14159265358979323846f * xr / c;
    const float t2 = t * t;
    const float f = t < 0.5f ? t * (-1.0f / 3.0f + t2 * (1.0f / 30.0f + t2 * (-1.0f / 840.0f + t2 * (1.0f / 45360.0f))))
                             : (t * cosf(t) - sinf(t)) / t2;
    return in ? sqrtf(2.0f / c) * sqrtf((float)n_basis) * a * a * f : 0.0f;
}

// part_small[wave slice][nb_pad*32 (dW0p) + N_MID*32*32 (dWm_p)]
// LEN: the adjoint w.r.t. the MLP's INPUT instead of its weights (matten_radial_mlp_bwd_len): the same recomputation, the
// same dw W2p^T stage and chain down to dz_0; then dL/demb = W0p dz_0 (one more matrix step, the D registers as the B
// operand again) and dlen[e] = sum_k dL/demb[k] b_k'(r_e).  No weight gradients, no h2 scratch, no partial sums.
template <int KS0, bool BF16, int N_MID, bool LEN = false>
__global__ __launch_bounds__(BW_WAVES * 64) void radial_mlp_bwd_edges(
    const float4* __restrict__ geom, int64_t E, int n_basis, float r_start, float r_end, const float* __restrict__ w0p,
    const float* __restrict__ w_mid, const float* __restrict__ w2p, int w_pad, int w_cols, const void* __restrict__ dw,
    int64_t dw_ld, float* __restrict__ h2_out, float* __restrict__ part_small, int tiles_per_wave, float s0, float s1,
    float* __restrict__ dlen = nullptr) {
    __shared__ float lds[BW_WAVES][(3 * HID + 16) * TS];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int g = lane >> 4, c = lane & 15;
    const int64_t slice = (int64_t)blockIdx.x * BW_WAVES + wave;
    const int64_t e_first = slice * (tiles_per_wave * 16);
    float* t_h1 = lds[wave];                 // [32][TS]  h1[k][e]
    float* t_dz2 = t_h1 + HID * TS;          // [32][TS]
    float* t_dz1 = t_dz2 + HID * TS;         // [32][TS]
    float* t_b = t_dz1 + HID * TS;           // [16][TS]  bessel[k0][e]
    // weights as matrix operands, fixed for the whole walk
    float a0[2][KS0], a1[nm1(N_MID)][2][8], a1t[nm1(N_MID)][2][8];
#pragma unroll
    for (int kk = 0; kk < KS0; ++kk) {
        a0[0][kk] = w0p[(4 * kk + g) * HID + c];
        a0[1][kk] = w0p[(4 * kk + g) * HID + 16 + c];
    }
#pragma unroll
    for (int m = 0; m < N_MID; ++m) {
        const float* __restrict__ w1p = w_mid + m * HID * HID;
#pragma unroll
        for (int kk = 0; kk < 8; ++kk) {
            const int k = 16 * (kk >> 2) + 4 * g + (kk & 3);    // pi(kk, g): the feature the lane's D register (kk) holds
            a1[m][0][kk] = w1p[k * HID + c];                     // forward:  A[m = out c][K = in k]
            a1[m][1][kk] = w1p[k * HID + 16 + c];
            a1t[m][0][kk] = w1p[c * HID + k];                    // adjoint:  A[m = in c][K = out k]
            a1t[m][1][kk] = w1p[(16 + c) * HID + k];
        }
    }
    float a0t[LEN ? 8 : 1];   // LEN: A[m = basis c][K = hidden pi(kk, g)] of dL/demb = W0p dz_0
    if constexpr (LEN) {
#pragma unroll
        for (int kk = 0; kk < 8; ++kk) a0t[kk] = c < 4 * KS0 ? w0p[c * HID + 16 * (kk >> 2) + 4 * g + (kk & 3)] : 0.0f;
    }
    // dWm_p[m-tile over in][n-tile over out] per middle layer, dW0p[n-tile over hidden] (rows = basis index)
    f32x4 g_w1[nm1(N_MID)][2][2], g_w0[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        g_w0[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int m = 0; m < nm1(N_MID); ++m)
#pragma unroll
            for (int j = 0; j < 2; ++j) g_w1[m][i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    for (int tile = 0; tile < tiles_per_wave; ++tile) {
        const int64_t e0 = e_first + tile * 16;
        if (e0 >= E) break;
        const int64_t e = e0 + c;
        const bool e_ok = e < E;
        const int64_t ec = e_ok ? e : E - 1;
        const float len = geom[ec].w;
        // ---- forward recomputation (same operand order as radial_mlp_kernel): z[i] of layer i, h[i] = silu(z[i]) the input
        // of middle layer i, h2 = silu(z[N_MID]) that of the last layer ----
        float bes[KS0];
        f32x4 z[N_MID + 1][2], h[nm1(N_MID)][2], h2[2];
#pragma unroll
        for (int i = 0; i <= N_MID; ++i) z[i][0] = z[i][1] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kk = 0; kk < KS0; ++kk) {
            const int k = 4 * kk + g;
            bes[kk] = (k < n_basis && e_ok) ? matten::bessel_basis(len, k, n_basis, r_start, r_end) : 0.0f;
            z[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[0][kk], bes[kk], z[0][0], 0, 0, 0);
            z[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[1][kk], bes[kk], z[0][1], 0, 0, 0);
        }
#pragma unroll
        for (int m = 0; m < N_MID; ++m) {
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) h[m][t][r] = silu(z[m][t][r]);
#pragma unroll
            for (int kk = 0; kk < 8; ++kk) {
                const float b = h[m][kk >> 2][kk & 3];
                z[m + 1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[m][0][kk], b, z[m + 1][0], 0, 0, 0);
                z[m + 1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[m][1][kk], b, z[m + 1][1], 0, 0, 0);
            }
        }
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) h2[t][r] = silu(z[N_MID][t][r]);
        if (!LEN && e_ok) {   // h2[e, 16 t + 4 g + r]: four consecutive floats per tile
            *reinterpret_cast<f32x4*>(h2_out + e * HID + 4 * g) = h2[0];
            *reinterpret_cast<f32x4*>(h2_out + e * HID + 16 + 4 * g) = h2[1];
        }
        // ---- dh2[k, e] = sum_q W2p[k, q] dw[e, q]: rows k = M, edges = N, columns q contracted 16 per load ----
        f32x4 dh2[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
        for (int q0 = 0; q0 < w_pad; q0 += 16) {
            const int q = q0 + 4 * g;
            f32x4 b4 = load4<BF16>(dw, ec * dw_ld + q);
            const f32x4 wa = *reinterpret_cast<const f32x4*>(w2p + (int64_t)c * w_pad + q);
            const f32x4 wb = *reinterpret_cast<const f32x4*>(w2p + (int64_t)(16 + c) * w_pad + q);
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const float b = (q + s < w_cols && e_ok) ? b4[s] : 0.0f;   // pad columns of dw are never written: select
                dh2[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[s], b, dh2[0], 0, 0, 0);
                dh2[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(wb[s], b, dh2[1], 0, 0, 0);
            }
        }
        // ---- dz_{i+1}, dh_i = Wm_i dz_{i+1} (contraction over the out index: the D registers are the B operand), ..., dz_0 ----
        f32x4 dz[N_MID + 1][2];
#pragma unroll
        for (int i = N_MID; i >= 0; --i) {
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) dz[i][t][r] = dh2[t][r] * dsilu(z[i][t][r]);
            if (i > 0) {
                dh2[0] = dh2[1] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int kk = 0; kk < 8; ++kk) {
                    const float b = dz[i][kk >> 2][kk & 3];
                    dh2[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1t[i > 0 ? i - 1 : 0][0][kk], b, dh2[0], 0, 0, 0);
                    dh2[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1t[i > 0 ? i - 1 : 0][1][kk], b, dh2[1], 0, 0, 0);
                }
            }
        }
        if constexpr (LEN) {
            // ---- dL/demb[k = 4 g + r][edge c], then this lane's four basis functions; the four lane groups add up ----
            f32x4 de = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kk = 0; kk < 8; ++kk)
                de = __builtin_amdgcn_mfma_f32_16x16x4f32(a0t[kk], dz[0][kk >> 2][kk & 3], de, 0, 0, 0);
            float dl = 0.0f;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int k = 4 * g + r;
                if (k < n_basis) dl = fmaf(de[r], bessel_basis_dr(len, k, n_basis, r_start, r_end), dl);
            }
            dl += __shfl_xor(dl, 16, 64);
            dl += __shfl_xor(dl, 32, 64);
            if (g == 0 && e_ok) dlen[e] = dl;
            continue;
        }
        // ---- the small weight gradients: contraction over the tile's 16 edges, operands through LDS ----
        small_grads_tile<KS0, N_MID>(t_h1, t_dz2, t_dz1, t_b, h, dz, bes, g, c, g_w1, g_w0);
        __builtin_amdgcn_wave_barrier();
    }
    if constexpr (LEN) return;
    const int nb_pad = 4 * KS0;
    store_small<KS0, N_MID>(part_small + slice * (int64_t)(nb_pad * HID + N_MID * HID * HID), g_w0, g_w1, g, c, s0, s1);
}

// ---- both halves in ONE kernel, dw read ONCE (w_pad <= 16 * 4 * FU_MAXCH) ---------------------------------------------
// radial_mlp_bwd_edges + radial_mlp_bwd_w2 stream dw[E, w_pad] twice and pass h2[E, 32] through memory.  Here a workgroup
// works in ROUNDS of four 16-edge tiles (tile t = wave t's tile of the round, the same edge assignment as above):
//   phase 0  wave t recomputes z1, h1, z2, h2 of tile t and publishes h2 to LDS ([tile][edge][k]: the A operand of dW2p)
//   phase A  the 16-column chunks of dw are dealt round-robin to the waves; for each of its chunks and each of the four
//            tiles a wave loads the 16 x 16 piece of dw once (16 bytes per lane, whole 64-byte pieces of 16 rows) and uses
//            it twice: as the B operand of dh2 += W2p dw^T (edges = N, as in radial_mlp_bwd_edges) and, transposed through
//            a wave-private LDS tile, of dW2p += h2^T dw (edges = the contraction).  The wave's dW2p columns stay in
//            registers for the whole walk (8 accumulator registers per chunk).
//   phase B  the four waves' partial dh2 of tile t are added in wave order by wave t (LDS), which then runs the rest of
//            the chain for its tile exactly as radial_mlp_bwd_edges does.
// Partial sums: part_small per wave (as above), part_w2 per WORKGROUP; fixed order, no atomics.
constexpr int FU_MAXCH = 8;                 // 16-column chunks per wave at most: w_pad <= 512
constexpr int FU_HS = HID + 1;              // row stride of the published h2 tiles
constexpr int FU_TT = 20;                   // row stride of the dw transpose tile (16-byte aligned rows)
constexpr int FU_POOL = BW_WAVES * 64 * 8;  // floats per wave of the shared pool: partial dh2 [tile][lane][8] / the phase-B tiles
static_assert((3 * HID + 16) * TS <= FU_POOL, "the phase-B transposes live in the wave's share of the pool");
template <int KS0, bool BF16, int MAXCH, int N_MID>
__global__ __launch_bounds__(BW_WAVES * 64, 2) void radial_mlp_bwd_fused(
    const float4* __restrict__ geom, int64_t E, int n_basis, float r_start, float r_end, const float* __restrict__ w0p,
    const float* __restrict__ w_mid, const float* __restrict__ w2p, int w_pad, int w_cols, const void* __restrict__ dw,
    int64_t dw_ld, float* __restrict__ part_small, float* __restrict__ part_w2, int tiles_per_wave, float s0, float s1,
    float s2) {
    // pool[wave]: the wave's partial dh2 [tile][lane][m, r] during phase A, its transposes in phase B (barrier between)
    __shared__ __attribute__((aligned(16))) float pool[BW_WAVES][FU_POOL];
    __shared__ float h2s[BW_WAVES][16 * FU_HS];                               // [tile][edge][k]
    __shared__ __attribute__((aligned(16))) float tts[BW_WAVES][16 * FU_TT];   // dw piece [edge][column] (per wave)
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int g = lane >> 4, c = lane & 15;
    const int64_t slice = (int64_t)blockIdx.x * BW_WAVES + wave;
    float* t_h1 = pool[wave];
    float* t_dz2 = t_h1 + HID * TS;
    float* t_dz1 = t_dz2 + HID * TS;
    float* t_b = t_dz1 + HID * TS;
    float* tt = tts[wave];
    // the small layers' weights as matrix operands: from LDS at every use (kept in registers they cost the kernel its
    // second wave per SIMD); 4 KB per middle layer
    __shared__ float w0s[16 * HID], wms[nm1(N_MID) * HID * HID];
    for (int i = threadIdx.x; i < 4 * KS0 * HID; i += BW_WAVES * 64) w0s[i] = w0p[i];
    for (int i = threadIdx.x; i < N_MID * HID * HID; i += BW_WAVES * 64) wms[i] = w_mid[i];
    __syncthreads();
    f32x4 g_w1[nm1(N_MID)][2][2], g_w0[2], g_w2[MAXCH][2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        g_w0[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int m = 0; m < nm1(N_MID); ++m)
#pragma unroll
            for (int j = 0; j < 2; ++j) g_w1[m][i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int j = 0; j < MAXCH; ++j) g_w2[j][0] = g_w2[j][1] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int n_chunks = w_pad >> 4;
    const int64_t wg_first = (int64_t)blockIdx.x * BW_WAVES * tiles_per_wave * 16;   // first edge of the workgroup
    for (int round = 0; round < tiles_per_wave; ++round) {
        if (wg_first + (int64_t)round * 16 >= E) break;   // uniform: not even wave 0 has a tile in this round
        // ---- phase 0: forward of this wave's tile (z1, h1, z2 are recomputed in phase B: held across phase A they cost
        // the registers that keep a second wave per SIMD) ----
        const int64_t e0 = (slice * tiles_per_wave + round) * 16;
        const int64_t e = e0 + c;
        const bool e_ok = e < E;
        const float len = geom[e_ok ? e : E - 1].w;
        // z[i] of layer i, h[i] = silu(z[i]) the input of middle layer i (as in radial_mlp_bwd_edges)
        auto forward_tile = [&](float (&bes)[KS0], f32x4 (&z)[N_MID + 1][2], f32x4 (&h)[nm1(N_MID)][2]) {
#pragma unroll
            for (int i = 0; i <= N_MID; ++i) z[i][0] = z[i][1] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kk = 0; kk < KS0; ++kk) {
                const int k = 4 * kk + g;
                bes[kk] = (k < n_basis && e_ok) ? matten::bessel_basis(len, k, n_basis, r_start, r_end) : 0.0f;
                z[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(w0s[k * HID + c], bes[kk], z[0][0], 0, 0, 0);
                z[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(w0s[k * HID + 16 + c], bes[kk], z[0][1], 0, 0, 0);
            }
#pragma unroll
            for (int m = 0; m < N_MID; ++m) {
                const float* w1s = wms + m * HID * HID;
#pragma unroll
                for (int t = 0; t < 2; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) h[m][t][r] = silu(z[m][t][r]);
#pragma unroll
                for (int kk = 0; kk < 8; ++kk) {
                    const float b = h[m][kk >> 2][kk & 3];
                    const int kf = 16 * (kk >> 2) + 4 * g + (kk & 3);   // pi(kk, g): the feature the lane's D register (kk) holds
                    z[m + 1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(w1s[kf * HID + c], b, z[m + 1][0], 0, 0, 0);
                    z[m + 1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(w1s[kf * HID + 16 + c], b, z[m + 1][1], 0, 0, 0);
                }
            }
        };
        // wide layers (more than 4 chunks per wave) recompute z, h in phase B: held across phase A they would spill;
        // narrow layers keep them (their phase A is short, the second evaluation would show: 0.20 vs 0.18 ms at 128 columns)
        // -- unless there is more than one middle layer to hold
        constexpr bool RECOMPUTE = MAXCH > 4 || N_MID > 1;
        float bes[KS0];
        f32x4 z[N_MID + 1][2], h[nm1(N_MID)][2];
        {
            float bes0[KS0];
            f32x4 za[N_MID + 1][2], ha[nm1(N_MID)][2];
            if constexpr (RECOMPUTE) forward_tile(bes0, za, ha);
            else forward_tile(bes, z, h);
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r)   // (0 for an edge past the end: its Bessel row is 0)
                    h2s[wave][c * FU_HS + 16 * t + 4 * g + r] = silu(RECOMPUTE ? za[N_MID][t][r] : z[N_MID][t][r]);
        }
        __syncthreads();
        // ---- phase A: this wave's column chunks over the round's four tiles ----
        f32x4 pdh[BW_WAVES][2];
#pragma unroll
        for (int t = 0; t < BW_WAVES; ++t) pdh[t][0] = pdh[t][1] = f32x4{0.f, 0.f, 0.f, 0.f};
        int64_t erow[BW_WAVES];
        bool eok[BW_WAVES];
#pragma unroll
        for (int t = 0; t < BW_WAVES; ++t) {
            const int64_t et = (((int64_t)blockIdx.x * BW_WAVES + t) * tiles_per_wave + round) * 16 + c;
            eok[t] = et < E;
            erow[t] = (eok[t] ? et : E - 1) * dw_ld;
        }
#pragma unroll
        for (int jj = 0; jj < MAXCH; ++jj) {
            const int j = jj * BW_WAVES + wave;
            if (j < n_chunks) {   // uniform over the wave
                const int q = 16 * j + 4 * g;
                f32x4 b4[BW_WAVES];
#pragma unroll
                for (int t = 0; t < BW_WAVES; ++t) b4[t] = load4<BF16>(dw, erow[t] + q);
                const f32x4 wa = *reinterpret_cast<const f32x4*>(w2p + (int64_t)c * w_pad + q);
                const f32x4 wb = *reinterpret_cast<const f32x4*>(w2p + (int64_t)(16 + c) * w_pad + q);
#pragma unroll
                for (int t = 0; t < BW_WAVES; ++t) {
                    f32x4 b = b4[t];
#pragma unroll
                    for (int sst = 0; sst < 4; ++sst) b[sst] = (q + sst < w_cols && eok[t]) ? b[sst] : 0.0f;   // pad columns of dw are never written: select
#pragma unroll
                    for (int sst = 0; sst < 4; ++sst) {
                        pdh[t][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[sst], b[sst], pdh[t][0], 0, 0, 0);
                        pdh[t][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(wb[sst], b[sst], pdh[t][1], 0, 0, 0);
                    }
                    // the same piece with the edges as the contraction: [edge c][column 4 g + s] -> [edge 4 s + g][column c]
                    *reinterpret_cast<f32x4*>(tt + c * FU_TT + 4 * g) = b;
                    __builtin_amdgcn_s_waitcnt(0xc07f);
                    __builtin_amdgcn_wave_barrier();
                    float bt[4];
#pragma unroll
                    for (int sst = 0; sst < 4; ++sst) bt[sst] = tt[(4 * sst + g) * FU_TT + c];
                    __builtin_amdgcn_wave_barrier();   // (the next piece's store follows these reads in the wave's LDS order)
#pragma unroll
                    for (int sst = 0; sst < 4; ++sst) {
                        // A operand of dW2p: h2[tile][edge 4 s + g][k = c + 16 m]
                        const float ha = h2s[t][(4 * sst + g) * FU_HS + c], hb = h2s[t][(4 * sst + g) * FU_HS + 16 + c];
                        g_w2[jj][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(ha, bt[sst], g_w2[jj][0], 0, 0, 0);
                        g_w2[jj][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(hb, bt[sst], g_w2[jj][1], 0, 0, 0);
                    }
                }
            }
        }
#pragma unroll
        for (int t = 0; t < BW_WAVES; ++t) {
            *reinterpret_cast<f32x4*>(&pool[wave][(t * 64 + lane) * 8]) = pdh[t][0];
            *reinterpret_cast<f32x4*>(&pool[wave][(t * 64 + lane) * 8 + 4]) = pdh[t][1];
        }
        __syncthreads();
        // ---- phase B: dh2 of this wave's tile (waves added in order), then the chain of radial_mlp_bwd_edges ----
        f32x4 dh2[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
#pragma unroll
        for (int w = 0; w < BW_WAVES; ++w) {
            dh2[0] += *reinterpret_cast<const f32x4*>(&pool[w][(wave * 64 + lane) * 8]);
            dh2[1] += *reinterpret_cast<const f32x4*>(&pool[w][(wave * 64 + lane) * 8 + 4]);
        }
        __syncthreads();   // every wave has its sums: the pool now takes the transposes
        if constexpr (RECOMPUTE) forward_tile(bes, z, h);
        f32x4 dz[N_MID + 1][2];
#pragma unroll
        for (int i = N_MID; i >= 0; --i) {
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) dz[i][t][r] = dh2[t][r] * dsilu(z[i][t][r]);
            if (i > 0) {
                const float* w1s = wms + (i > 0 ? i - 1 : 0) * HID * HID;
                dh2[0] = dh2[1] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int kk = 0; kk < 8; ++kk) {
                    const float b = dz[i][kk >> 2][kk & 3];
                    const int kf = 16 * (kk >> 2) + 4 * g + (kk & 3);
                    dh2[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(w1s[c * HID + kf], b, dh2[0], 0, 0, 0);
                    dh2[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(w1s[(16 + c) * HID + kf], b, dh2[1], 0, 0, 0);
                }
            }
        }
        small_grads_tile<KS0, N_MID>(t_h1, t_dz2, t_dz1, t_b, h, dz, bes, g, c, g_w1, g_w0);
        __syncthreads();   // the next round overwrites h2s / dh2p
    }
    const int nb_pad = 4 * KS0;
    store_small<KS0, N_MID>(part_small + slice * (int64_t)(nb_pad * HID + N_MID * HID * HID), g_w0, g_w1, g, c, s0, s1);
    // dW2p[k = 16 m + 4 g + r][column 16 j + c] of this workgroup
    float* out2 = part_w2 + (int64_t)blockIdx.x * HID * w_pad;
#pragma unroll
    for (int jj = 0; jj < MAXCH; ++jj) {
        const int j = jj * BW_WAVES + wave;
        if (j < n_chunks) {
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int r = 0; r < 4; ++r) out2[(int64_t)(16 * m + 4 * g + r) * w_pad + 16 * j + c] = g_w2[jj][m][r] * s2;
        }
    }
}

// part_w2[range][32][w_pad]; grid = (ceil(w_pad / 64), n_ranges), wave w of a block owns columns [64 bx + 16 w, +16)
template <bool BF16>
__global__ __launch_bounds__(BW_WAVES * 64) void radial_mlp_bwd_w2(const float* __restrict__ h2, const void* __restrict__ dw,
                                                                  int64_t dw_ld, int64_t E, int w_pad,
                                                                  float* __restrict__ part_w2, int range, float s2) {
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int g = lane >> 4, c = lane & 15;
    const int q0 = (blockIdx.x * BW_WAVES + wave) * 16;
    if (q0 >= w_pad) return;
    const int64_t e_beg = (int64_t)blockIdx.y * range;
    const int64_t e_end = min(E, e_beg + range);
    f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    for (int64_t e0 = e_beg; e0 < e_end; e0 += 16) {
        float a[4][2], b[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {   // K step s: edge e0 + 4 s + g; A[m = k][K = edge] = h2[edge][k], B[K = edge][n = q]
            const int64_t e = e0 + 4 * s + g;
            const bool ok = e < e_end;
            const int64_t ec = ok ? e : e_end - 1;
            a[s][0] = ok ? h2[ec * HID + c] : 0.0f;
            a[s][1] = ok ? h2[ec * HID + 16 + c] : 0.0f;
            b[s] = ok ? load1<BF16>(dw, ec * dw_ld + q0 + c) : 0.0f;
        }
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s][0], b[s], acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s][1], b[s], acc[1], 0, 0, 0);
        }
    }
    float* out = part_w2 + (int64_t)blockIdx.y * HID * w_pad;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) out[(int64_t)(16 * t + 4 * g + r) * w_pad + q0 + c] = acc[t][r] * s2;
}

// out[i] = sum over the n partial rows part[s][i] in a FIXED order: a workgroup owns RED_COLS columns, its RED_GROUPS thread
// groups take every RED_GROUPS-th row each (sequentially), and group 0 adds the group sums in group order.  grid.y = 0: the
// small gradients, 1: dW2.  (16 columns x 64 groups: with ~1000 partial rows -- radial_mlp_bwd_w2 cuts the edges into as
// many ranges as fill the chip -- a thread adds 16 rows instead of 64: the kernel is a chain of dependent loads.)
constexpr int RED_COLS = 16, RED_GROUPS = 64;
__global__ __launch_bounds__(RED_COLS * RED_GROUPS) void radial_mlp_bwd_reduce(const float* __restrict__ part_small, int64_t n_small,
                                                              int small_len, const float* __restrict__ part_w2,
                                                              int64_t n_rng, int w2_len, float* __restrict__ out_small,
                                                              float* __restrict__ out_w2) {
    __shared__ float red[RED_GROUPS][RED_COLS];
    const float* part = blockIdx.y ? part_w2 : part_small;
    const int64_t n = blockIdx.y ? n_rng : n_small;
    const int len = blockIdx.y ? w2_len : small_len;
    float* out = blockIdx.y ? out_w2 : out_small;
    const int lc = threadIdx.x % RED_COLS, grp = threadIdx.x / RED_COLS;
    const int col = blockIdx.x * RED_COLS + lc;
    if (blockIdx.x * RED_COLS >= len) return;
    float v = 0.0f;
    if (col < len)
        for (int64_t s = grp; s < n; s += RED_GROUPS) v += part[s * len + col];
    red[grp][lc] = v;
    __syncthreads();
    if (grp == 0 && col < len) {
        float t = red[0][lc];
#pragma unroll 8
        for (int gq = 1; gq < RED_GROUPS; ++gq) t += red[gq][lc];
        out[col] = t;
    }
}

}  // namespace

extern "C" int64_t matten_radial_mlp_bwd_small_slices(int64_t n_edges) {
    return matten_cdiv(matten_cdiv(n_edges, bw_tiles(n_edges) * 16), BW_WAVES) * BW_WAVES;
}
// one kernel (dw read once) where the wave's share of dW2p fits its registers
#ifndef BW_FUSED
#define BW_FUSED 1
#endif
#ifndef BW_FUSED_MIN_W
#define BW_FUSED_MIN_W 128   // narrower layers: too few column chunks for four waves (48 columns: 0.16 vs 0.13 ms at 293 k edges)
#endif
// column chunks per wave the one-kernel adjoint takes without scratch, by the number of middle layers (their weight
// gradients and recomputed activations take the registers of dW2p's chunks; 1: the shipped shape, as before)
constexpr int fu_maxch(int n_mid) { return n_mid == 1 ? FU_MAXCH : (n_mid == 0 ? 6 : (n_mid == 2 ? 4 : 0)); }
static inline bool bw_fused(int64_t w_pad, int n_mid) {
    return BW_FUSED && w_pad >= BW_FUSED_MIN_W && w_pad <= 16 * BW_WAVES * fu_maxch(n_mid);
}
// partial rows of dW2p: one per workgroup of the fused kernel, else one per edge range of radial_mlp_bwd_w2
extern "C" int64_t matten_radial_mlp_bwd_w2_ranges_deep(int64_t n_edges, int64_t w_pad, int n_mid) {
    if (bw_fused(w_pad, n_mid)) return matten_radial_mlp_bwd_small_slices(n_edges) / BW_WAVES;
    return matten_cdiv(n_edges, w2_range(n_edges, w_pad));
}
extern "C" int64_t matten_radial_mlp_bwd_w2_ranges(int64_t n_edges, int64_t w_pad) {
    return matten_radial_mlp_bwd_w2_ranges_deep(n_edges, w_pad, 1);
}

// the one-kernel adjoint at the smallest chunk count that covers w_pad; only the (N_MID, chunks) pairs bw_fused admits
// are instantiated
template <int K, bool B, int NM>
static void launch_bwd_fused(unsigned grid1, hipStream_t stream, const float* geom_sorted, int64_t n_edges, int n_basis,
                             float r_start, float r_end, const float* w0p, const float* w_mid, const float* w2p, int w_pad,
                             int w_cols, const void* dw, int64_t dw_ld, float* part_small, float* part_w2, float scale0,
                             float scale1, float scale2) {
#define LAUNCH_FUSED_M(M)                                                                                              \
    radial_mlp_bwd_fused<K, B, M, NM><<<grid1, BW_WAVES * 64, 0, stream>>>((const float4*)geom_sorted, n_edges, n_basis, \
                                                                           r_start, r_end, w0p, w_mid, w2p, w_pad, w_cols, \
                                                                           dw, dw_ld, part_small, part_w2,                 \
                                                                           bw_tiles(n_edges), scale0, scale1, scale2)
    if constexpr (fu_maxch(NM) >= 4) {
        if (w_pad <= 16 * BW_WAVES * 4) { LAUNCH_FUSED_M(4); return; }
    }
    if constexpr (fu_maxch(NM) >= 6) {
        if (w_pad <= 16 * BW_WAVES * 6) { LAUNCH_FUSED_M(6); return; }
    }
    if constexpr (fu_maxch(NM) >= FU_MAXCH) LAUNCH_FUSED_M(FU_MAXCH);
#undef LAUNCH_FUSED_M
}

static int radial_mlp_bwd_launch(const float* geom_sorted, int64_t n_edges, int n_basis, float r_start, float r_end,
                                 const float* w0p, int nb_pad, const float* w_mid, int n_mid, const float* w2p, int hidden,
                                 int w_pad, int w_cols, const void* dw, int64_t dw_ld, int dw_is_bf16, float* h2_scratch,
                                 float* part_small, float* part_w2, float scale0, float scale1, float scale2,
                                 float* grad_small, float* grad_w2, matten_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (n_edges < 0 || hidden != HID || (w_pad & 15) || w_pad <= 0 || w_cols <= 0 || w_cols > w_pad || (nb_pad & 3) ||
        nb_pad < n_basis || nb_pad > 16 || dw_ld < w_pad || (dw_ld & 3) || n_mid < 0 || n_mid > MATTEN_RADIAL_MAX_MID)
        return MATTEN_EINVAL;
    if (n_edges == 0) return MATTEN_OK;
    if (!geom_sorted || !w0p || (n_mid > 0 && !w_mid) || !w2p || !dw || !h2_scratch || !part_small || !part_w2)
        return MATTEN_EINVAL;
    const unsigned grid1 = (unsigned)(matten_radial_mlp_bwd_small_slices(n_edges) / BW_WAVES);
    const bool fused = bw_fused(w_pad, n_mid);
#define LAUNCH_FUSED(K, B, NM)                                                                                          \
    launch_bwd_fused<K, B, NM>(grid1, stream, geom_sorted, n_edges, n_basis, r_start, r_end, w0p, w_mid, w2p, w_pad, w_cols, \
                               dw, dw_ld, part_small, part_w2, scale0, scale1, scale2)
#define LAUNCH(K, B, NM) if (fused) LAUNCH_FUSED(K, B, NM); else                                                          \
    radial_mlp_bwd_edges<K, B, NM><<<grid1, BW_WAVES * 64, 0, stream>>>((const float4*)geom_sorted, n_edges, n_basis,     \
                                                                     r_start, r_end, w0p, w_mid, w2p, w_pad, w_cols, dw, \
                                                                     dw_ld, h2_scratch, part_small, bw_tiles(n_edges), scale0, scale1)
#define LAUNCH_NM(K, B)                   \
    switch (n_mid) {                      \
        case 0: LAUNCH(K, B, 0); break;   \
        case 1: LAUNCH(K, B, 1); break;   \
        case 2: LAUNCH(K, B, 2); break;   \
        default: LAUNCH(K, B, 3); break;  \
    }
#define LAUNCH_K(B)                       \
    switch (nb_pad >> 2) {                \
        case 1: LAUNCH_NM(1, B); break;   \
        case 2: LAUNCH_NM(2, B); break;   \
        case 3: LAUNCH_NM(3, B); break;   \
        default: LAUNCH_NM(4, B); break;  \
    }
    if (dw_is_bf16) { LAUNCH_K(true) } else { LAUNCH_K(false) }
#undef LAUNCH_K
#undef LAUNCH_NM
#undef LAUNCH
#undef LAUNCH_FUSED
    MATTEN_LAUNCH_CHECK();
    dim3 grid2((unsigned)matten_cdiv(w_pad, 16 * BW_WAVES),
               (unsigned)matten_radial_mlp_bwd_w2_ranges_deep(n_edges, w_pad, n_mid));
    if (fused) {
    } else if (dw_is_bf16)
        radial_mlp_bwd_w2<true><<<grid2, BW_WAVES * 64, 0, stream>>>(h2_scratch, dw, dw_ld, n_edges, w_pad, part_w2,
                                                                     w2_range(n_edges, w_pad), scale2);
    else
        radial_mlp_bwd_w2<false><<<grid2, BW_WAVES * 64, 0, stream>>>(h2_scratch, dw, dw_ld, n_edges, w_pad, part_w2,
                                                                      w2_range(n_edges, w_pad), scale2);
    MATTEN_LAUNCH_CHECK();
    if (grad_small || grad_w2) {   // the final, ordered sums in the same call (both or neither)
        if (!grad_small || !grad_w2) return MATTEN_EINVAL;
        const int small_len = nb_pad * HID + n_mid * HID * HID, w2_len = HID * w_pad;
        radial_mlp_bwd_reduce<<<dim3((unsigned)matten_cdiv(std::max(small_len, w2_len), RED_COLS), 2), RED_COLS * RED_GROUPS, 0, stream>>>(
            part_small, matten_radial_mlp_bwd_small_slices(n_edges), small_len, part_w2,
            matten_radial_mlp_bwd_w2_ranges_deep(n_edges, w_pad, n_mid), w2_len, grad_small, grad_w2);
        MATTEN_LAUNCH_CHECK();
    }
    return MATTEN_OK;
}

extern "C" int matten_radial_mlp_bwd(const float* geom_sorted, int64_t n_edges, int n_basis, float r_start, float r_end,
                                     const float* w0p, int nb_pad, const float* w1p, const float* w2p, int hidden,
                                     int w_pad, int w_cols, const void* dw, int64_t dw_ld, int dw_is_bf16,
                                     float* h2_scratch, float* part_small, float* part_w2, float scale0, float scale1,
                                     float scale2, float* grad_small, float* grad_w2, matten_stream_t stream_) {
    if (!w1p && n_edges > 0) return MATTEN_EINVAL;
    return radial_mlp_bwd_launch(geom_sorted, n_edges, n_basis, r_start, r_end, w0p, nb_pad, w1p, 1, w2p, hidden, w_pad,
                                 w_cols, dw, dw_ld, dw_is_bf16, h2_scratch, part_small, part_w2, scale0, scale1, scale2,
                                 grad_small, grad_w2, stream_);
}

extern "C" int matten_radial_mlp_bwd_deep(const float* geom_sorted, int64_t n_edges, int n_basis, float r_start,
                                          float r_end, const float* w0p, int nb_pad, const float* w_mid, int n_mid,
                                          const float* w2p, int hidden, int w_pad, int w_cols, const void* dw,
                                          int64_t dw_ld, int dw_is_bf16, float* h2_scratch, float* part_small,
                                          float* part_w2, float scale0, float scale1, float scale2, float* grad_small,
                                          float* grad_w2, matten_stream_t stream_) {
    return radial_mlp_bwd_launch(geom_sorted, n_edges, n_basis, r_start, r_end, w0p, nb_pad, w_mid, n_mid, w2p, hidden,
                                 w_pad, w_cols, dw, dw_ld, dw_is_bf16, h2_scratch, part_small, part_w2, scale0, scale1,
                                 scale2, grad_small, grad_w2, stream_);
}

// adjoint w.r.t. the edge length: radial_mlp_bwd_edges in its LEN form, every depth through one entry
extern "C" int matten_radial_mlp_bwd_len(const float* geom_sorted, int64_t n_edges, int n_basis, float r_start, float r_end,
                                         const float* w0p, int nb_pad, const float* w_mid, int n_mid, const float* w2p,
                                         int hidden, int w_pad, int w_cols, const void* dw, int64_t dw_ld, int dw_is_bf16,
                                         float* dlen, matten_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (n_edges < 0 || hidden != HID || (w_pad & 15) || w_pad <= 0 || w_cols <= 0 || w_cols > w_pad || (nb_pad & 3) ||
        nb_pad < n_basis || nb_pad <= 0 || nb_pad > 16 || dw_ld < w_pad || (dw_ld & 3) || n_mid < 0 ||
        n_mid > MATTEN_RADIAL_MAX_MID)
        return MATTEN_EINVAL;
    if (n_edges == 0) return MATTEN_OK;
    if (!geom_sorted || !w0p || (n_mid > 0 && !w_mid) || !w2p || !dw || !dlen) return MATTEN_EINVAL;
    const unsigned grid1 = (unsigned)(matten_radial_mlp_bwd_small_slices(n_edges) / BW_WAVES);
#define LAUNCH(K, B, NM)                                                                                                  \
    radial_mlp_bwd_edges<K, B, NM, true><<<grid1, BW_WAVES * 64, 0, stream>>>(                                            \
        (const float4*)geom_sorted, n_edges, n_basis, r_start, r_end, w0p, w_mid, w2p, w_pad, w_cols, dw, dw_ld, nullptr, \
        nullptr, bw_tiles(n_edges), 1.0f, 1.0f, dlen)
#define LAUNCH_NM(K, B)                   \
    switch (n_mid) {                      \
        case 0: LAUNCH(K, B, 0); break;   \
        case 1: LAUNCH(K, B, 1); break;   \
        case 2: LAUNCH(K, B, 2); break;   \
        default: LAUNCH(K, B, 3); break;  \
    }
#define LAUNCH_K(B)                       \
    switch (nb_pad >> 2) {                \
        case 1: LAUNCH_NM(1, B); break;   \
        case 2: LAUNCH_NM(2, B); break;   \
        case 3: LAUNCH_NM(3, B); break;   \
        default: LAUNCH_NM(4, B); break;  \
    }
    if (dw_is_bf16) { LAUNCH_K(true) } else { LAUNCH_K(false) }
#undef LAUNCH_K
#undef LAUNCH_NM
#undef LAUNCH
    MATTEN_LAUNCH_CHECK();
    return MATTEN_OK;
}

// (w0 [nb,32], w1 [N_MID,32,32], w2 [32,W] raw parameters) -> the packed operands of matten_radial_mlp / _bwd in ONE
// launch: w0p [nb_pad,32] = s0 w0 (zero rows past nb), w1p = s1 w1, w2p [32,w_pad] = s2 w2 (zero columns past W).
namespace {
template <int N_MID>
__global__ void radial_pack_kernel(const float* __restrict__ w0, const float* __restrict__ w1, const float* __restrict__ w2,
                                   int nb, int nb_pad, int W, int w_pad, float s0, float s1, float s2,
                                   float* __restrict__ w0p, float* __restrict__ w1p, float* __restrict__ w2p) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int n0 = nb_pad * HID, n1 = N_MID * HID * HID, n2 = HID * w_pad;
    if (i < n0) {
        w0p[i] = (i / HID) < nb ? w0[i] * s0 : 0.0f;
    } else if (i < n0 + n1) {
        w1p[i - n0] = w1[i - n0] * s1;
    } else if (i < n0 + n1 + n2) {
        const int j = i - n0 - n1, k = j / w_pad, q = j - k * w_pad;
        w2p[j] = q < W ? w2[k * W + q] * s2 : 0.0f;
    }
}
}  // namespace

static int radial_pack_launch(const float* w0, const float* w1, int n_mid, const float* w2, int n_basis, int nb_pad,
                              int w_cols, int w_pad, float scale0, float scale1, float scale2, float* w0p, float* w1p,
                              float* w2p, matten_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (n_basis <= 0 || nb_pad < n_basis || w_cols <= 0 || w_pad < w_cols || n_mid < 0 || n_mid > MATTEN_RADIAL_MAX_MID)
        return MATTEN_EINVAL;
    if (!w0 || (n_mid > 0 && (!w1 || !w1p)) || !w2 || !w0p || !w2p) return MATTEN_EINVAL;
    const int n = nb_pad * HID + n_mid * HID * HID + HID * w_pad;
#define LAUNCH(M)                                                                                                      \
    radial_pack_kernel<M><<<(unsigned)matten_cdiv(n, 256), 256, 0, stream>>>(w0, w1, w2, n_basis, nb_pad, w_cols, w_pad, \
                                                                            scale0, scale1, scale2, w0p, w1p, w2p)
    switch (n_mid) {
        case 0: LAUNCH(0); break;
        case 1: LAUNCH(1); break;
        case 2: LAUNCH(2); break;
        default: LAUNCH(3); break;
    }
#undef LAUNCH
    MATTEN_LAUNCH_CHECK();
    return MATTEN_OK;
}

extern "C" int matten_radial_pack(const float* w0, const float* w1, const float* w2, int n_basis, int nb_pad, int w_cols,
                                  int w_pad, float scale0, float scale1, float scale2, float* w0p, float* w1p, float* w2p,
                                  matten_stream_t stream_) {
    if (!w1 || !w1p) return MATTEN_EINVAL;
    return radial_pack_launch(w0, w1, 1, w2, n_basis, nb_pad, w_cols, w_pad, scale0, scale1, scale2, w0p, w1p, w2p, stream_);
}

extern "C" int matten_radial_pack_deep(const float* w0, const float* w_mid, int n_mid, const float* w2, int n_basis,
                                       int nb_pad, int w_cols, int w_pad, float scale0, float scale1, float scale2,
                                       float* w0p, float* w_mid_p, float* w2p, matten_stream_t stream_) {
    return radial_pack_launch(w0, w_mid, n_mid, w2, n_basis, nb_pad, w_cols, w_pad, scale0, scale1, scale2, w0p, w_mid_p,
                              w2p, stream_);
}

// ---- operands of matten_tp_fused derived from the RAW radial layers by kernels (training on the production kernel: the
// parameters change every step, the inference path's cached library-op derivations would run every step) --------------
namespace {

// as radial_pack_kernel, the last layer's columns gathered through `cols` (fused column order; -1 = structural zero)
template <int N_MID>
__global__ void radial_pack_cols_kernel(const float* __restrict__ w0, const float* __restrict__ w1,
                                        const float* __restrict__ w2, int nb, int nb_pad, int W,
                                        const int64_t* __restrict__ cols, int n_cols, int w_pad, float s0, float s1, float s2,
                                        float* __restrict__ w0p, float* __restrict__ w1p, float* __restrict__ w2p) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int n0 = nb_pad * HID, n1 = N_MID * HID * HID, n2 = HID * w_pad;
    if (i < n0) {
        w0p[i] = (i / HID) < nb ? w0[i] * s0 : 0.0f;
    } else if (i < n0 + n1) {
        w1p[i - n0] = w1[i - n0] * s1;
    } else if (i < n0 + n1 + n2) {
        const int j = i - n0 - n1, k = j / w_pad, q = j - k * w_pad;
        const int64_t src = q < n_cols ? cols[q] : -1;
        w2p[j] = src >= 0 ? w2[(int64_t)k * W + src] * s2 : 0.0f;
    }
}

// [s, 1 / s]: the power of two the last hidden features are multiplied by so that |s h| < 2^15 for every edge length
// (nn/utils.py RadialMLP._fp16_scale, same bound: |h| <= sqrt(2/c) sqrt(nb) pi / c * n0 * n_1 ... n_{N_MID} with the
// column-sum norms n0 = max_col sum_k |W0[k,col]| (k+1) / sqrt(nb), n_i = max_col sum_k |Wm_i[k,col]| act_cst / sqrt(h))
template <int N_MID>
__global__ void radial_h_scale_kernel(const float* __restrict__ w0, const float* __restrict__ w1, int nb, float c,
                                      float act_cst, float* __restrict__ out) {
    __shared__ float red[1 + N_MID][HID];
    const int col = threadIdx.x;   // 32 threads
    float a0 = 0.0f;
    for (int k = 0; k < nb; ++k) a0 += fabsf(w0[k * HID + col]) * (float)(k + 1);
    red[0][col] = a0 / sqrtf((float)nb);
#pragma unroll
    for (int m = 0; m < N_MID; ++m) {
        float a1 = 0.0f;
        for (int k = 0; k < HID; ++k) a1 += fabsf(w1[m * HID * HID + k * HID + col]);
        red[1 + m][col] = a1 * (act_cst / sqrtf((float)HID));
    }
    __syncthreads();
    if (col == 0) {
        float n0 = 0.0f;
        for (int i = 0; i < HID; ++i) n0 = fmaxf(n0, red[0][i]);
        float bound = sqrtf(2.0f / c) * sqrtf((float)nb) * 3.141592653589793f / c * n0;
#pragma unroll
        for (int m = 0; m < N_MID; ++m) {
            float n1 = 0.0f;
            for (int i = 0; i < HID; ++i) n1 = fmaxf(n1, red[1 + m][i]);
            bound = bound * n1;
        }
        float s = 1.0f;
        if (bound > 32768.0f) s = exp2f(floorf(log2f(16384.0f / fmaxf(bound, 1e-30f))));
        if (!(s > 0.0f) || isinf(s) || isnan(s)) s = exp2f(-100.0f);
        out[0] = s;
        out[1] = 1.0f / s;
    }
}

// group entries' weight blocks as the fp16 hi / lo MFMA fragments matten_tp_fused consumes (same values as
// ops.split_a_tiles): per entry a power-of-two scale that puts its largest magnitude in [2^13, 2^14).
// frag[(a_tile + mt) * 64 + lane][16 halves: hi(kk 0..7) | lo(kk 0..7)], lane = 16 g + c:
//   value = W2p[pi(kk, g)][w_base + 16 mt + c] * scale,  pi(kk, g) = 16 (kk >> 2) + 4 g + (kk & 3)
// scale_inv[entry] = 2^-(scale exponent) * h_scale_inv
__global__ void split_a_tiles_kernel(const float* __restrict__ w2p, int w_pad, const int32_t* __restrict__ entries,
                                     const float* __restrict__ h_scale, _Float16* __restrict__ frag,
                                     float* __restrict__ scale_inv) {
    __shared__ float red[256];
    const int e = blockIdx.x;
    const int32_t* ge = entries + (int64_t)e * 32;
    const int w_base = ge[5], a_tile = ge[6], n_mt = ge[7];
    const int ncol = 16 * n_mt;
    float amax = 0.0f;
    for (int i = threadIdx.x; i < HID * ncol; i += blockDim.x) {
        const int k = i / ncol, q = i - k * ncol;
        if (w_base + q < w_pad) amax = fmaxf(amax, fabsf(w2p[(int64_t)k * w_pad + w_base + q]));   // (a tile may reach past the last column)
    }
    red[threadIdx.x] = amax;
    __syncthreads();
    for (int o = blockDim.x / 2; o > 0; o >>= 1) {
        if (threadIdx.x < o) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + o]);
        __syncthreads();
    }
    amax = red[0];
    int ex = (int)((__float_as_uint(amax) >> 23) & 0xffu) - 127;
    ex = amax > 0.0f ? max(-100, min(100, ex)) : 13;
    const float sc = __uint_as_float((unsigned)(127 + 13 - ex) << 23);
    if (threadIdx.x == 0) scale_inv[e] = __uint_as_float((unsigned)(127 - 13 + ex) << 23) * (h_scale ? h_scale[1] : 1.0f);
    const float tiny = 6.103515625e-05f;
    for (int i = threadIdx.x; i < n_mt * 64; i += blockDim.x) {
        const int mt = i >> 6, lane = i & 63, g = lane >> 4, c = lane & 15;
        _Float16* dst = frag + ((int64_t)(a_tile + mt) * 64 + lane) * 16;
#pragma unroll
        for (int kk = 0; kk < 8; ++kk) {
            const int k = 16 * (kk >> 2) + 4 * g + (kk & 3);
            const int col = w_base + 16 * mt + c;
            const float v = col < w_pad ? w2p[(int64_t)k * w_pad + col] * sc : 0.0f;
            const float hi = fabsf(v) < tiny ? 0.0f : (float)(_Float16)v;
            float lo = (v - hi) * 2048.0f;
            lo = fabsf(lo) < tiny ? 0.0f : lo;
            dst[kk] = (_Float16)hi;
            dst[8 + kk] = (_Float16)lo;
        }
    }
}

}  // namespace

static int radial_pack_cols_launch(const float* w0, const float* w1, int n_mid, const float* w2, int n_basis, int nb_pad,
                                   int w_cols, const int64_t* cols, int n_cols, int w_pad, float scale0, float scale1,
                                   float scale2, float* w0p, float* w1p, float* w2p, matten_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (n_basis <= 0 || nb_pad < n_basis || w_cols <= 0 || n_cols <= 0 || w_pad < n_cols || n_mid < 0 ||
        n_mid > MATTEN_RADIAL_MAX_MID)
        return MATTEN_EINVAL;
    if (!w0 || (n_mid > 0 && (!w1 || !w1p)) || !w2 || !cols || !w0p || !w2p) return MATTEN_EINVAL;
    const int n = nb_pad * HID + n_mid * HID * HID + HID * w_pad;
#define LAUNCH(M)                                                                                                            \
    radial_pack_cols_kernel<M><<<(unsigned)matten_cdiv(n, 256), 256, 0, stream>>>(w0, w1, w2, n_basis, nb_pad, w_cols, cols, \
                                                                                  n_cols, w_pad, scale0, scale1, scale2, w0p, \
                                                                                  w1p, w2p)
    switch (n_mid) {
        case 0: LAUNCH(0); break;
        case 1: LAUNCH(1); break;
        case 2: LAUNCH(2); break;
        default: LAUNCH(3); break;
    }
#undef LAUNCH
    MATTEN_LAUNCH_CHECK();
    return MATTEN_OK;
}

extern "C" int matten_radial_pack_cols(const float* w0, const float* w1, const float* w2, int n_basis, int nb_pad, int w_cols,
                                       const int64_t* cols, int n_cols, int w_pad, float scale0, float scale1, float scale2,
                                       float* w0p, float* w1p, float* w2p, matten_stream_t stream_) {
    if (!w1 || !w1p) return MATTEN_EINVAL;
    return radial_pack_cols_launch(w0, w1, 1, w2, n_basis, nb_pad, w_cols, cols, n_cols, w_pad, scale0, scale1, scale2, w0p,
                                   w1p, w2p, stream_);
}

extern "C" int matten_radial_pack_cols_deep(const float* w0, const float* w_mid, int n_mid, const float* w2, int n_basis,
                                            int nb_pad, int w_cols, const int64_t* cols, int n_cols, int w_pad, float scale0,
                                            float scale1, float scale2, float* w0p, float* w_mid_p, float* w2p,
                                            matten_stream_t stream_) {
    return radial_pack_cols_launch(w0, w_mid, n_mid, w2, n_basis, nb_pad, w_cols, cols, n_cols, w_pad, scale0, scale1, scale2,
                                   w0p, w_mid_p, w2p, stream_);
}

static int radial_h_scale_launch(const float* w0, const float* w1, int n_mid, int n_basis, float r_start, float r_end,
                                 float act_cst, float* out2, matten_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (n_basis <= 0 || !(r_end > r_start) || !w0 || (n_mid > 0 && !w1) || !out2 || n_mid < 0 ||
        n_mid > MATTEN_RADIAL_MAX_MID)
        return MATTEN_EINVAL;
#define LAUNCH(M) radial_h_scale_kernel<M><<<1, HID, 0, stream>>>(w0, w1, n_basis, r_end - r_start, act_cst, out2)
    switch (n_mid) {
        case 0: LAUNCH(0); break;
        case 1: LAUNCH(1); break;
        case 2: LAUNCH(2); break;
        default: LAUNCH(3); break;
    }
#undef LAUNCH
    MATTEN_LAUNCH_CHECK();
    return MATTEN_OK;
}

extern "C" int matten_radial_h_scale(const float* w0, const float* w1, int n_basis, float r_start, float r_end, float act_cst,
                                     float* out2, matten_stream_t stream_) {
    if (!w1) return MATTEN_EINVAL;
    return radial_h_scale_launch(w0, w1, 1, n_basis, r_start, r_end, act_cst, out2, stream_);
}

extern "C" int matten_radial_h_scale_deep(const float* w0, const float* w_mid, int n_mid, int n_basis, float r_start,
                                          float r_end, float act_cst, float* out2, matten_stream_t stream_) {
    return radial_h_scale_launch(w0, w_mid, n_mid, n_basis, r_start, r_end, act_cst, out2, stream_);
}

extern "C" int matten_split_a_tiles(const float* w2p, int64_t w_pad, const int32_t* group_entries, int64_t n_entries,
                                    const float* h_scale, uint16_t* frag, float* scale_inv, matten_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (n_entries <= 0 || w_pad <= 0 || !w2p || !group_entries || !frag || !scale_inv) return MATTEN_EINVAL;
    split_a_tiles_kernel<<<(unsigned)n_entries, 256, 0, stream>>>(w2p, (int)w_pad, group_entries, h_scale, (_Float16*)frag,
                                                                 scale_inv);
    MATTEN_LAUNCH_CHECK();
    return MATTEN_OK;
}
