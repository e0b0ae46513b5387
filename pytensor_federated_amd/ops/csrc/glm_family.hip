// Single-chain GLM families on CDNA4 (gfx950): k_glm_family and its C entry
// point fed_glm_family.  Shared pieces and the overview of the GLM units are
// in fed_common.hpp; the wave-per-row logistic kernel this one generalises
// is in glm_logistic.hip.
//
// Why a second single-chain kernel.  k_logistic_glm_reg gives a whole wave
// to one row, so the feature dimension is padded to WAVE*VEC (512 bf16 /
// 256 f32).  Count and multi-covariate Gaussian regressions are usually
// narrow (K ~ 20): padded to a wave they would read 25x their data.  Here a
// GROUP of G <= 64 lanes owns a row and a wave handles R = 64/G consecutive
// rows per step.  With K = G*VEC the row stride equals the group's span, so
// lane l of a step reads bytes [16*l, 16*l+16) of ONE contiguous 1 KiB
// segment: the same fully coalesced access at every G, and X is read once
// at its own size.  At G = 64 (and KITER > 1 chunks of 64*VEC columns) the
// layout is exactly the wave-per-row kernel's.
//
// What turns z = x.beta (+ offset) into a logp term and a residual is the
// link, a compile-time policy (glm_links.hpp, shared with the batched kernel):
//   Poisson  (log link)   term = y*z - exp(z)         resid = y - exp(z)
//   Gaussian (identity)   term = -r*r/(2 sigma^2)     resid = r/sigma^2, r = y-z
//   Logistic              the expressions of k_logistic_glm_reg, in its order
// y and offset are always f32: counts above 256 do not survive bf16, and
// they are N elements against N*K.  logp_const (the part of logp that does
// not depend on beta) is added on the device by block 0, so out[] is final
// with no extra launch and no host synchronisation.
//
// Reductions.  z: xor butterfly over the group's lanes (every lane of the
// group ends with the full sum).  grad: each lane keeps gacc[KITER][VEC]
// (statically indexed) for its own columns over all its rows; lanes with
// equal lane % G are summed once at the end, then waves are summed in LDS
// and the block writes one fp32 slab row, reduced by the shared
// k_colsum_reduce.  logp: fp64 per group leader.
//
// Ragged steps.  Rows at or past n_rows are zero-filled by a conditional
// load (the clamped-address form spills, see TODO.md) and masked out of
// BOTH logp and the residual: a zero row is not inert for every link
// (Poisson: exp(0) = 1).
//
// Registers.  gfx950 ISA of all 54 instantiations (3 links x 2 dtypes x
// {G = 1..64, KITER = 2, 4}) checked with
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -S --cuda-device-only \
//         -Rpass-analysis=kernel-resource-usage glm_family.hip
// every one reports ScratchSize 0 and no VGPR/SGPR spill.  VGPRs by
// (dtype, KITER): bf16 42-80 / 92-124 / 155-220, f32 30-63 / 60-80 / 92-108;
// bf16 KITER = 4 holds 128 data registers, as in k_logistic_glm_reg (178
// VGPRs there), occupancy 2-3.
// No inline assembly.  Measurements: profiles/PROFILES.md "GLM family kernel".

#include "fed_common.hpp"
#include "glm_links.hpp"
#include "row_group.hpp"

// sum over the G lanes of a group; every lane of the group gets the total
template <int G>
__device__ __forceinline__ float group_allreduce_f32(float v) {
#pragma unroll
    for (int off = G / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, WAVE);
    return v;
}

template <typename T, int G, int KITER, class Link>  // K = KITER*G*VEC; KITER > 1 only at G = 64
__global__ __launch_bounds__(256) void k_glm_family(
    const T* __restrict__ X,            // [N][K] row-major
    const float* __restrict__ y,        // [N]
    const float* __restrict__ offset,   // [N] or NULL
    long long n_rows,
    const float* __restrict__ beta,     // [K]
    LinkParams lp,
    double logp_const,
    double* __restrict__ logp_out,      // pre-zeroed scalar
    float* __restrict__ grad_slab       // [gridDim][K]
) {
    using TR = VecTraits<T>;
    constexpr int VEC = TR::VEC;
    constexpr int R = WAVE / G;          // rows per step
    constexpr int CHUNK = G * VEC;       // columns per c iteration
    constexpr int K = KITER * CHUNK;
    static_assert(KITER == 1 || G == WAVE, "column chunks only in the wave-per-row layout");
    const int lane = threadIdx.x & (WAVE - 1);
    const int wid = threadIdx.x / WAVE;
    const int waves_per_block = blockDim.x / WAVE;
    const long long wave_id = (long long)blockIdx.x * waves_per_block + wid;
    const long long n_waves = (long long)gridDim.x * waves_per_block;
    const int grp = lane / G;            // which of the step's R rows
    const int sub = lane % G;            // lane within the group
    const int col0 = sub * VEC;          // first column of this lane in chunk 0

    float xa[KITER][VEC];                // this lane's slice of step s
    float xb[KITER][VEC];                // ... and of step s+1
    float breg[KITER][VEC];              // this lane's beta slice (loop-invariant)
    float gacc[KITER][VEC];              // this lane's grad accumulator
#pragma unroll
    for (int c = 0; c < KITER; ++c)
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            breg[c][j] = beta[c * CHUNK + col0 + j];
            gacc[c][j] = 0.f;
        }

    double logp_acc = 0.0;
    // Two steps per iteration: both steps' global loads issue before either
    // step's dependent dot/reduce/transcendental chain, so each wave keeps
    // ~2x the HBM traffic in flight (the reason glm_logistic.hip gives: its
    // 1-row loop measured 68% of HBM peak, the dependent chain was the gap).
    const long long pair_stride = n_waves * 2;
    long long s = wave_id * 2;
    for (; (s + 2) * R <= n_rows; s += pair_stride) {
        const long long ra = s * R + grp;
        const long long rb = ra + R;
        const T* pa = X + ra * (long long)K + col0;
        const T* pb = pa + (long long)R * K;
#pragma unroll
        for (int c = 0; c < KITER; ++c) {
            // nontemporal: each X row is consumed once (from registers for
            // both logp and grad) -- do not displace L2/L3 lines
            const u32x4_t va = __builtin_nontemporal_load((const u32x4_t*)(pa + c * CHUNK));
            const u32x4_t vb = __builtin_nontemporal_load((const u32x4_t*)(pb + c * CHUNK));
            TR::unpack(va, xa[c]);
            TR::unpack(vb, xb[c]);
        }
        const float ya = __builtin_nontemporal_load(y + ra);
        const float yb = __builtin_nontemporal_load(y + rb);
        float za = 0.f, zb = 0.f;
        if (offset) {  // wave-uniform
            za = __builtin_nontemporal_load(offset + ra);
            zb = __builtin_nontemporal_load(offset + rb);
        }
        float zap = 0.f, zbp = 0.f;
#pragma unroll
        for (int c = 0; c < KITER; ++c)
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                zap += xa[c][j] * breg[c][j];
                zbp += xb[c][j] * breg[c][j];
            }
        za += group_allreduce_f32<G>(zap);
        zb += group_allreduce_f32<G>(zbp);
        float ta, tb, resa, resb;
        Link::eval(ya, za, lp, ta, resa);
        Link::eval(yb, zb, lp, tb, resb);
        if (sub == 0) logp_acc += (double)ta + (double)tb;
#pragma unroll
        for (int c = 0; c < KITER; ++c)
#pragma unroll
            for (int j = 0; j < VEC; ++j)
                gacc[c][j] += resa * xa[c][j] + resb * xb[c][j];
    }
    // what is left of this wave's last pair: at most two steps, of which the
    // last may be ragged
    for (int t = 0; t < 2; ++t) {
        const long long row = (s + t) * R + grp;
        if ((s + t) * R >= n_rows) break;  // wave-uniform
        const bool valid = row < n_rows;
        const T* pr = X + row * (long long)K + col0;
#pragma unroll
        for (int c = 0; c < KITER; ++c) {
            u32x4_t v = {0u, 0u, 0u, 0u};
            if (valid) v = __builtin_nontemporal_load((const u32x4_t*)(pr + c * CHUNK));
            TR::unpack(v, xa[c]);
        }
        float yr = 0.f, z = 0.f;
        if (valid) {
            yr = y[row];
            if (offset) z = offset[row];
        }
        float zp = 0.f;
#pragma unroll
        for (int c = 0; c < KITER; ++c)
#pragma unroll
            for (int j = 0; j < VEC; ++j) zp += xa[c][j] * breg[c][j];
        z += group_allreduce_f32<G>(zp);
        float term, resid;
        Link::eval(yr, z, lp, term, resid);
        if (!valid) resid = 0.f;
        if (sub == 0 && valid) logp_acc += (double)term;
#pragma unroll
        for (int c = 0; c < KITER; ++c)
#pragma unroll
            for (int j = 0; j < VEC; ++j) gacc[c][j] += resid * xa[c][j];
    }

    // The block epilogue below (fold, LDS sum, slab row) is written out in
    // k_logistic_glm_reg (its G = 64 case) and k_glm_family_fvp as well.  A
    // shared __forceinline__ helper was tried and withdrawn: the compiler
    // simplifies a helper on its own before inlining it, and the ISA of all 54
    // instantiations here moved (block order, the waves_per_block guard no
    // longer shared with the logp loop, 2 SGPRs in two of them): see
    // profiles/PROFILES.md "Row-group glue".

    // lanes with equal lane % G hold partials of the same columns
#pragma unroll
    for (int c = 0; c < KITER; ++c)
#pragma unroll
        for (int j = 0; j < VEC; ++j)
#pragma unroll
            for (int off = WAVE / 2; off >= G; off >>= 1)
                gacc[c][j] += __shfl_xor(gacc[c][j], off, WAVE);

    // cross-wave grad reduction in LDS (dynamic: K floats), then one slab row
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* g_lds = reinterpret_cast<float*>(smem);                           // [K]
    double* l_lds = reinterpret_cast<double*>(smem + ((K * 4 + 15) & ~15));  // [waves]
    for (int w = 0; w < waves_per_block; ++w) {
        if (wid == w && lane < G) {
#pragma unroll
            for (int c = 0; c < KITER; ++c)
#pragma unroll
                for (int j = 0; j < VEC; ++j) {
                    const int col = c * CHUNK + col0 + j;
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

    const double wave_logp = wave_reduce_sum(logp_acc);  // non-leaders hold 0
    if (lane == 0) l_lds[wid] = wave_logp;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = blockIdx.x == 0 ? logp_const : 0.0;
        for (int w = 0; w < waves_per_block; ++w) t += l_lds[w];
        atomicAdd(logp_out, t);
    }
}

extern "C" {

// out = fp64[1+K] = {logp, grad...}; beta_f32 = fp32[K] device; y_f32 and
// offset_f32 (may be NULL) = fp32[n_rows] device; workspace holds the fp32
// grad slab (ws_bytes >= grid*K*4).  K = G*VEC for G in {1,...,64}, or
// KITER*64*VEC for KITER in {2, 4}.  Returns -2 bad dtype, -3 workspace too
// small, -4 unsupported K, -5 unknown link.
int fed_glm_family(
    const void* X, const float* y_f32, const float* offset_f32,
    long long n_rows, int K, const float* beta_f32, int link,
    double sigma, double logp_const,
    double* out, float* workspace, long long ws_bytes,
    int dtype, void* stream_v
) {
    hipStream_t stream = (hipStream_t)stream_v;
    RowGroupPlan plan;
    if (const int bad = plan_row_group(dtype, link, K, n_rows, ws_bytes, plan)) return bad;
    const int grid = plan.grid, block = plan.block;
    const int lds_bytes = ((K * 4 + 15) & ~15) + block / WAVE * 8;

    hipError_t err = hipMemsetAsync(out, 0, (1 + K) * sizeof(double), stream);
    if (err != hipSuccess) return (int)err;

    const LinkParams lp = make_link_params(sigma);
    const int rc = dispatch_row_group(dtype, link, K, [&](auto t, auto l, auto g, auto kiter) {
        using T = typename decltype(t)::type;
        using Link = typename decltype(l)::type;
        hipLaunchKernelGGL((k_glm_family<T, decltype(g)::value, decltype(kiter)::value, Link>),
                           dim3(grid), dim3(block), lds_bytes, stream, (const T*)X, y_f32,
                           offset_f32, n_rows, beta_f32, lp, logp_const, out, workspace);
    });
    if (rc != 0) return rc;
    hipError_t kerr = hipGetLastError();
    if (kerr != hipSuccess) return (int)kerr;

    return launch_colsum_reduce(workspace, grid, K, out + 1, stream);
}

}  // extern "C"
