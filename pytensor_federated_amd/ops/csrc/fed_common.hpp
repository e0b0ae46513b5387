// CDNA4 (gfx950 / MI355X) fused logp+grad kernels for the federated GLM
// worker models.  Hand-written HIP -- no hipify, no CUDA compatibility.
//
// Replaces the reference's PyTensor-compiled worker functions
// (reference demo_node.py:30-43: pytensor.function([a,b],[logp,*grads]))
// with single-pass, wave64-tiled reductions:
//
//  * fed_gaussian_linear: r = y-(a+b*x); logp, dlogp/da, dlogp/db in ONE
//    pass over x,y (3 reductions fused; HBM-bound, ~4 B/row traffic).
//  * fed_logistic_glm:    z = X.beta row-dot, p = sigmoid(z),
//    logp += y*z - softplus(z), grad += (y-p)*X_row -- X is read EXACTLY
//    once for both logp and grad (the row stays in registers between the
//    dot and the rank-1 grad update).  Per-block grad partials go to a
//    deterministic fp32 slab, reduced by a second tiny kernel.
//
// Numerics: bf16/f32 inputs accumulate fp32 per lane over short spans,
// fp64 across lanes/waves/blocks; f64 inputs accumulate fp64 throughout.
// Outputs are fp64 device buffers shaped for direct RCCL all-reduce:
// [logp, grads...] (the wire layout of common.wrap_logp_grad_func).
//
// Build: hipcc --offload-arch=gfx950 -O3 -shared -fPIC (see ops/build.py).
//
// This header holds what the GLM translation units share (dtype plumbing,
// reductions, sc1 accessors, grid sizing, the slab reduce kernel):
//   glm_gaussian.hip          fused Gaussian kernel, shard engine, server
//   glm_logistic.hip          single-chain logistic kernel
//   glm_logistic_batched.hip  16-chain MFMA logistic kernels
//   glm_family.hip            row-group single-chain kernel, link as a policy
//                             (Poisson, Gaussian on K covariates, logistic)
//   glm_family_batched.hip    16-chain MFMA kernel for the Poisson and Gaussian
//                             links (the link policies are in glm_links.hpp)
//   glm_family_fisher.hip     Fisher information X^T diag(w) X of the Poisson and
//                             Gaussian links on the matrix cores
//   glm_family_fvp.hip        Fisher-vector product X^T (w * (X v)) and diag(H)
//                             of all three links, one pass in the row-group
//                             geometry

#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdlib.h>

#define WAVE 64

// ---------------------------------------------------------------------------
// dtype plumbing
// ---------------------------------------------------------------------------

__device__ __forceinline__ float bf16_bits_to_f32(unsigned short u) {
    union { unsigned int i; float f; } cvt;
    cvt.i = ((unsigned int)u) << 16;
    return cvt.f;
}

// 16-byte vector loads: 8 bf16 / 4 f32 / 2 f64 per lane per instruction
// (G13: hipcc does not auto-vectorize bf16 loads; scalar bf16 is ~2x slower).
struct U4 { unsigned int x, y, z, w; };
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4_t;

template <typename T> struct VecTraits;
template <> struct VecTraits<float> {
    static constexpr int VEC = 4;
    using acc_t = float;
    __device__ static inline void load(const float* p, float* out) {
        const float4 v = *reinterpret_cast<const float4*>(p);
        out[0] = v.x; out[1] = v.y; out[2] = v.z; out[3] = v.w;
    }
    __device__ static inline float get(const float* p, long long i) { return p[i]; }
    __device__ static inline void unpack(const u32x4_t v, float* out) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            union { unsigned int u; float f; } c;
            c.u = v[j];
            out[j] = c.f;
        }
    }
};
template <> struct VecTraits<double> {
    static constexpr int VEC = 2;
    using acc_t = double;
    __device__ static inline void load(const double* p, double* out) {
        const double2 v = *reinterpret_cast<const double2*>(p);
        out[0] = v.x; out[1] = v.y;
    }
    __device__ static inline double get(const double* p, long long i) { return p[i]; }
    __device__ static inline void unpack(const u32x4_t v, double* out) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            union { unsigned long long u; double d; } c;
            c.u = ((unsigned long long)v[2 * j + 1] << 32) | v[2 * j];
            out[j] = c.d;
        }
    }
};
struct bf16_tag { unsigned short bits; };
template <> struct VecTraits<bf16_tag> {
    static constexpr int VEC = 8;
    using acc_t = float;
    __device__ static inline void load(const bf16_tag* p, float* out) {
        const U4 v = *reinterpret_cast<const U4*>(p);
        const unsigned int w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            out[2 * j]     = bf16_bits_to_f32((unsigned short)(w[j] & 0xffffu));
            out[2 * j + 1] = bf16_bits_to_f32((unsigned short)(w[j] >> 16));
        }
    }
    __device__ static inline float get(const bf16_tag* p, long long i) {
        return bf16_bits_to_f32(p[i].bits);
    }
    __device__ static inline void unpack(const u32x4_t v, float* out) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            out[2 * j]     = bf16_bits_to_f32((unsigned short)(v[j] & 0xffffu));
            out[2 * j + 1] = bf16_bits_to_f32((unsigned short)(v[j] >> 16));
        }
    }
};

// ---------------------------------------------------------------------------
// cross-lane / cross-wave reduction helpers (wave64!)
// ---------------------------------------------------------------------------

__device__ __forceinline__ double wave_reduce_sum(double v) {
#pragma unroll
    for (int off = WAVE / 2; off > 0; off >>= 1) {
        v += __shfl_down(v, off, WAVE);
    }
    return v;  // valid in lane 0 of the wave
}

__device__ __forceinline__ float wave_reduce_sum_f32(float v) {
#pragma unroll
    for (int off = WAVE / 2; off > 0; off >>= 1) {
        v += __shfl_down(v, off, WAVE);
    }
    return v;
}

// Agent-scope write-through (sc1) accessors for cross-workgroup slabs
// (G16 R1's cheap form: sc1 stores + drained ticket on the producer, sc1
// loads on the consumer -- no release/acquire fences, which cost ~1.7 us
// per block and made a fence-based combine 2.7x slower than two kernels).
typedef __attribute__((address_space(1))) unsigned long long gu64_t;
typedef __attribute__((address_space(1))) unsigned gu32_t;

__device__ __forceinline__ void store_sc1_f64(double* p, double v) {
    union { double d; unsigned long long u; } c;
    c.d = v;
    __hip_atomic_store((gu64_t*)p, c.u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ double load_sc1_f64(const double* p) {
    union { unsigned long long u; double d; } c;
    c.u = __hip_atomic_load((const gu64_t*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return c.d;
}

// Block-level fp64 reduction of NACC per-lane values via LDS; the block's
// totals land in lane 0 of wave 0.  BLOCK = 256 threads = 4 waves.
template <int NACC>
__device__ inline void block_reduce_add(double* vals, double* lds /* [4][NACC] */) {
    const int lane = threadIdx.x & (WAVE - 1);
    const int wid = threadIdx.x / WAVE;
#pragma unroll
    for (int k = 0; k < NACC; ++k) {
        const double w = wave_reduce_sum(vals[k]);
        if (lane == 0) lds[wid * NACC + k] = w;
    }
    __syncthreads();
    if (wid == 0) {
#pragma unroll
        for (int k = 0; k < NACC; ++k) {
            double total = 0.0;
            if (lane == 0) {
#pragma unroll
                for (int w = 0; w < 4; ++w) total += lds[w * NACC + k];
            }
            vals[k] = total;
        }
    }
}

// Column-wise fp64 reduction of the grad slab into out[1..K].
// grid = (ceil(K/256), CHUNKS): blockIdx.y sums a slice of the slab rows and
// fp64-atomicAdds its column partials (CHUNKS atomics per address -- cheap;
// a 1-d grid is latency-bound: 4 blocks reading 8 MB measured 363 us).
// inline: the single-chain and batched units both launch it, and each links
// its own copy (no -fgpu-rdc).  clang warns that CUDA would ignore the
// keyword on a kernel; HIP honours it (the symbol comes out weak).
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wcuda-compat"
inline __global__ __launch_bounds__(256) void k_colsum_reduce(
    const float* __restrict__ slab,  // [n_slabs][K]
    int n_slabs,
    int K,
    double* __restrict__ out_grad  // [K], pre-zeroed
) {
    const int col = blockIdx.x * blockDim.x + threadIdx.x;
    if (col >= K) return;
    const int chunk = (n_slabs + gridDim.y - 1) / gridDim.y;
    const int b0 = blockIdx.y * chunk;
    const int b1 = min(b0 + chunk, n_slabs);
    double s = 0.0;
    for (int b = b0; b < b1; ++b) s += (double)slab[(long long)b * K + col];
    if (gridDim.y == 1)
        out_grad[col] = s;
    else
        atomicAdd(&out_grad[col], s);
}
#pragma clang diagnostic pop

// ---------------------------------------------------------------------------
// host-side helpers shared by the C entry points
// ---------------------------------------------------------------------------

enum FedDtype { FED_F32 = 0, FED_F64 = 1, FED_BF16 = 2 };

static inline int grid_cap(void) {
    static int cap = 0;
    if (cap == 0) {
        const char* env = getenv("FED_GRID_CAP");
        cap = env ? atoi(env) : 1024;  // G11: cap + grid-stride (A/B on MI355X: 512-1024 best)
        if (cap < 1 || cap > 8192) cap = 2048;
    }
    return cap;
}

static inline int pick_grid(long long work_items, int block) {
    long long blocks = (work_items + block - 1) / block;
    if (blocks > grid_cap()) blocks = grid_cap();
    if (blocks < 1) blocks = 1;
    return (int)blocks;
}

// Sum the fp32 slab [n_slabs][cols] into out[cols] with k_colsum_reduce: one
// y-chunk of the grid per 8 slab rows, 1..64 of them.  `out` must already be
// zeroed (with more than one chunk the kernel accumulates by atomics); the
// memset stays with the caller, whose main kernel may have added into `out`
// after it.  Returns hipGetLastError().
static inline int launch_colsum_reduce(const float* slab, int n_slabs, int cols, double* out,
                                       hipStream_t stream) {
    int chunks = n_slabs / 8;
    if (chunks < 1) chunks = 1;
    if (chunks > 64) chunks = 64;
    hipLaunchKernelGGL(k_colsum_reduce, dim3((cols + 255) / 256, chunks), dim3(256), 0, stream,
                       slab, n_slabs, cols, out);
    return (int)hipGetLastError();
}
