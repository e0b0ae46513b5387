// Single-chain logistic GLM on CDNA4 (gfx950): k_logistic_glm_reg and its C
// entry point.  Shared pieces and the overview of the GLM units are in
// fed_common.hpp; the 16-chain MFMA kernels are in glm_logistic_batched.hip.

#include "fed_common.hpp"

// ---------------------------------------------------------------------------
// Logistic GLM: fused z = X.beta, logp, grad = X^T (y - sigmoid(z))
// ---------------------------------------------------------------------------
//
// One WAVE owns one row at a time (grid-stride over rows).  The row's
// feature chunk assignments: iteration c covers columns
// [c*WAVE*VEC, (c+1)*WAVE*VEC); lane l holds columns c*WAVE*VEC + l*VEC + j.
// For K <= KMAX_REG (held in registers) the row is loaded once and reused
// for the grad update; larger K falls back to a second (L2-hot) read.
//
// Per-block grad partials: each wave accumulates its lanes' column slices
// in registers across all its rows, then waves are summed in LDS and the
// block writes one fp32 slab row: slab[block][K].  k_colsum_reduce sums the
// slab into out[1..K] (deterministic; no fp32 global atomics).

template <typename T, int KITER>  // KITER = K / (WAVE*VEC), compile-time
__global__ __launch_bounds__(256) void k_logistic_glm_reg(
    const T* __restrict__ X,   // [N][K] row-major
    const T* __restrict__ y,
    long long n_rows,
    int K,
    const float* __restrict__ beta,  // [K]
    double* __restrict__ logp_out,   // pre-zeroed scalar
    float* __restrict__ grad_slab    // [gridDim][K]
) {
    using TR = VecTraits<T>;
    constexpr int VEC = TR::VEC;
    const int lane = threadIdx.x & (WAVE - 1);
    const int wid = threadIdx.x / WAVE;
    const int waves_per_block = blockDim.x / WAVE;
    const long long wave_id = (long long)blockIdx.x * waves_per_block + wid;
    const long long n_waves = (long long)gridDim.x * waves_per_block;

    // per-lane register state
    float xreg[KITER][VEC];        // this lane's row slice
    float breg[KITER][VEC];        // this lane's beta slice (loop-invariant)
    float gacc[KITER][VEC];        // this lane's grad accumulator
#pragma unroll
    for (int c = 0; c < KITER; ++c)
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            breg[c][j] = beta[c * WAVE * VEC + lane * VEC + j];
            gacc[c][j] = 0.f;
        }

    double logp_acc = 0.0;
    // Two rows per iteration: both rows' global loads issue before either
    // row's dependent dot/reduce/transcendental chain, so each wave keeps
    // ~2x the HBM traffic in flight (the 1-row loop measured 68% of HBM
    // peak; the dependent per-row chain was the gap).
    float xreg2[KITER][VEC];
    const long long pair_stride = n_waves * 2;
    long long r = wave_id * 2;
    for (; r + 1 < n_rows; r += pair_stride) {
        const T* row0 = X + r * (long long)K;
        const T* row1 = row0 + K;
        float z0p = 0.f, z1p = 0.f;
#pragma unroll
        for (int c = 0; c < KITER; ++c) {
            // nontemporal: each X row is consumed once (from registers for
            // both logp and grad) -- do not displace L2/L3 lines
            const u32x4_t v0 = __builtin_nontemporal_load(
                (const u32x4_t*)(row0 + c * WAVE * VEC + lane * VEC));
            const u32x4_t v1 = __builtin_nontemporal_load(
                (const u32x4_t*)(row1 + c * WAVE * VEC + lane * VEC));
            TR::unpack(v0, xreg[c]);
            TR::unpack(v1, xreg2[c]);
        }
#pragma unroll
        for (int c = 0; c < KITER; ++c)
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                z0p += xreg[c][j] * breg[c][j];
                z1p += xreg2[c][j] * breg[c][j];
            }
        float z0 = wave_reduce_sum_f32(z0p);
        float z1 = wave_reduce_sum_f32(z1p);
        z0 = __shfl(z0, 0, WAVE);
        z1 = __shfl(z1, 0, WAVE);
        const float y0 = TR::get(y, r);
        const float y1 = TR::get(y, r + 1);
        // stable: y*z - softplus(z) = y*z - (max(z,0) + log1p(exp(-|z|)))
        const float sp0 = fmaxf(z0, 0.f) + log1pf(__expf(-fabsf(z0)));
        const float sp1 = fmaxf(z1, 0.f) + log1pf(__expf(-fabsf(z1)));
        if (lane == 0) logp_acc += (double)(y0 * z0 - sp0) + (double)(y1 * z1 - sp1);
        const float res0 = y0 - 1.f / (1.f + __expf(-z0));
        const float res1 = y1 - 1.f / (1.f + __expf(-z1));
#pragma unroll
        for (int c = 0; c < KITER; ++c)
#pragma unroll
            for (int j = 0; j < VEC; ++j)
                gacc[c][j] += res0 * xreg[c][j] + res1 * xreg2[c][j];
    }
    for (; r < n_rows; r += pair_stride) {  // odd tail row of this wave
        const T* row = X + r * (long long)K;
        float z_part = 0.f;
#pragma unroll
        for (int c = 0; c < KITER; ++c) {
            TR::load(row + c * WAVE * VEC + lane * VEC, xreg[c]);
#pragma unroll
            for (int j = 0; j < VEC; ++j) z_part += xreg[c][j] * breg[c][j];
        }
        float z = wave_reduce_sum_f32(z_part);
        z = __shfl(z, 0, WAVE);
        const float yr = TR::get(y, r);
        const float sp = fmaxf(z, 0.f) + log1pf(__expf(-fabsf(z)));
        if (lane == 0) logp_acc += (double)(yr * z - sp);
        const float resid = yr - 1.f / (1.f + __expf(-z));
#pragma unroll
        for (int c = 0; c < KITER; ++c)
#pragma unroll
            for (int j = 0; j < VEC; ++j) gacc[c][j] += resid * xreg[c][j];
    }

    // cross-wave grad reduction in LDS (dynamic: K floats), then one slab row
    // (the G = 64 case of k_glm_family's epilogue; why it is a copy: note there)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* g_lds = reinterpret_cast<float*>(smem);                  // [K]
    double* l_lds = reinterpret_cast<double*>(smem + ((K * 4 + 15) & ~15));  // [waves]
    for (int w = 0; w < waves_per_block; ++w) {
        if (wid == w) {
#pragma unroll
            for (int c = 0; c < KITER; ++c)
#pragma unroll
                for (int j = 0; j < VEC; ++j) {
                    const int col = c * WAVE * VEC + lane * VEC + j;
                    if (w == 0)
                        g_lds[col] = gacc[c][j];
                    else
                        g_lds[col] += gacc[c][j];
                }
        }
        __syncthreads();
    }
    float* slab_row = grad_slab + (long long)blockIdx.x * K;
    for (int col = threadIdx.x; col < K; col += blockDim.x) slab_row[col] = g_lds[col];

    if (lane == 0) l_lds[wid] = logp_acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int w = 0; w < waves_per_block; ++w) t += l_lds[w];
        atomicAdd(logp_out, t);
    }
}

extern "C" {

// out = fp64[1+K] = {logp, grad...}; beta_f32 = fp32[K] device;
// workspace holds the fp32 grad slab (ws_bytes >= grid*K*4).
int fed_logistic_glm(
    const void* X, const void* y, long long n_rows, int K,
    const float* beta_f32,
    double* out, float* workspace, long long ws_bytes,
    int dtype, void* stream_v
) {
    hipStream_t stream = (hipStream_t)stream_v;
    hipError_t err = hipMemsetAsync(out, 0, (1 + K) * sizeof(double), stream);
    if (err != hipSuccess) return (int)err;
    const int block = 256;
    const int waves_per_block = block / WAVE;
    int grid = pick_grid(n_rows / waves_per_block + 1, 1);
    if (grid > 1024) grid = 1024;
    const long long need = (long long)grid * K * sizeof(float);
    if (need > ws_bytes) grid = (int)(ws_bytes / ((long long)K * sizeof(float)));
    if (grid < 1) return -3;
    const int lds_bytes = ((K * 4 + 15) & ~15) + waves_per_block * 8;

#define LAUNCH_LOGISTIC(T, KITER)                                                      \
    hipLaunchKernelGGL((k_logistic_glm_reg<T, KITER>), dim3(grid), dim3(block),        \
                       lds_bytes, stream, (const T*)X, (const T*)y, n_rows, K,         \
                       beta_f32, out, workspace)

    if (dtype == FED_BF16) {
        switch (K) {
            case 512:  LAUNCH_LOGISTIC(bf16_tag, 1); break;
            case 1024: LAUNCH_LOGISTIC(bf16_tag, 2); break;
            case 2048: LAUNCH_LOGISTIC(bf16_tag, 4); break;
            default: return -4;  // K must be a multiple of 512 (wave64 x bf16x8)
        }
    } else if (dtype == FED_F32) {
        switch (K) {
            case 256:  LAUNCH_LOGISTIC(float, 1); break;
            case 512:  LAUNCH_LOGISTIC(float, 2); break;
            case 1024: LAUNCH_LOGISTIC(float, 4); break;
            default: return -4;
        }
    } else {
        return -2;
    }
#undef LAUNCH_LOGISTIC
    hipError_t kerr = hipGetLastError();
    if (kerr != hipSuccess) return (int)kerr;

    return launch_colsum_reduce(workspace, grid, K, out + 1, stream);
}

}  // extern "C"
