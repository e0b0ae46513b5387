// Fisher-vector product of the GLM families on CDNA4 (gfx950):
// k_glm_family_fvp and its C entry point fed_glm_family_fvp.
//
//   out = X^T (w(z) * (X v)),   z = X beta (+ offset),   w = Link::weight(z)
//
// the product of the Fisher information H = X^T diag(w) X (glm_family_fisher.hip
// forms it whole on the matrix cores) with one vector, in ONE pass over X and
// without a K x K object: what a conjugate-gradient Newton step needs.  With
// no v the same kernel accumulates w * x * x, the diagonal of H (the Jacobi
// preconditioner).  No weight depends on y, so y is not read.
//
// Geometry: k_glm_family's (glm_family.hip), unchanged.  A group of G <= 64
// lanes owns a row, a wave handles R = 64/G consecutive rows per step, every
// lane loads one 16-byte nontemporal vector per column chunk, K = G*VEC or
// KITER*64*VEC (KITER in {2, 4}), two steps per loop iteration so that both
// steps' loads are in flight before either step's dependent chain (one shape
// excepted, see "Registers").  The row stays in registers between the two
// dots (x.beta and x.v, formed from the same registers) and the rank-1
// update acc += (w * u) * x, u = x.v.
//
// Reductions.  x.beta and x.v, of both rows of the pair: ONE reduction over
// the group's lanes that carries all four values, so the shuffles of the
// independent sums interleave instead of forming dependent chains, and the
// halves of a group share them (group_allreduce4_f32 below).
// acc: as k_glm_family's grad -- lanes with equal lane % G are summed once at
// the end, waves are summed in LDS, the block writes one fp32 slab row and the
// shared k_colsum_reduce adds the slab rows in fp64.
//
// Ragged steps.  Rows at or past n_rows are zero-filled by the conditional
// load and their weight is forced to 0: a zero row is not inert (Poisson:
// exp(0) = 1, and the diagonal has no u = 0 to hide behind).
//
// Diagonal mode is a wave-uniform branch on v == NULL, not a template flag:
// the instantiations stay at 54, and the branch is taken once per step.
//
// Registers.  gfx950 ISA of all 54 instantiations (3 links x 2 dtypes x
// {G = 1..64, KITER = 2, 4}) checked with
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -S --cuda-device-only \
//         -Rpass-analysis=kernel-resource-usage glm_family_fvp.hip
// every one reports ScratchSize 0, no VGPR/SGPR spill and no AGPR.  VGPRs by
// (dtype, KITER): bf16 44-72 / 114-120 / 174-177, f32 32-55 / 68-72 / 116-120.
// bf16 KITER = 4 runs ONE step per iteration: v adds 32 loop-invariant
// registers to k_glm_family's 128 data registers, and with both steps' slices
// held the compiler reported 256 VGPRs plus 20-22 AGPRs used as spill space
// (Poisson, logistic; occupancy 1).  One step at a time holds 128 data
// registers again, occupancy 2 as k_glm_family has at its widest.
// No inline assembly.  Measurements: profiles/PROFILES.md "GLM Fisher-vector
// kernel".

#include "fed_common.hpp"
#include "glm_links.hpp"
#include "row_group.hpp"

// Sums over the G lanes of a group of several independent values at once;
// every lane of the group gets the totals.  A plain xor butterfly moves every
// value at every stride (log2 G shuffles per value, 24 for the four values of
// a pair of steps at G = 64, and the shuffles are what a step waits for).
// Here a stride's two halves of the group share the work instead: at the
// widest stride each lane hands the half of the values its partner keeps and
// adds what it receives to the half it keeps, so every later stride moves
// half as many values; once a lane holds one value it runs the butterfly's
// remaining strides on it, and the totals travel back over the same strides.
// Four values: log2 G + 4 shuffles (10 at G = 64), two values: log2 G + 1.
// Every total is formed once and copied, so the lanes of a group agree bit for
// bit, as they do after a butterfly.
template <int G>
__device__ __forceinline__ void group_allreduce2_f32(float& a, float& b) {
    if constexpr (G >= 2) {
        const bool hi = (threadIdx.x & (G / 2)) != 0;
        float keep = (hi ? b : a) + __shfl_xor(hi ? a : b, G / 2, WAVE);
#pragma unroll
        for (int off = G / 4; off > 0; off >>= 1) keep += __shfl_xor(keep, off, WAVE);
        const float other = __shfl_xor(keep, G / 2, WAVE);
        a = hi ? other : keep;
        b = hi ? keep : other;
    }
}

template <int G>
__device__ __forceinline__ void group_allreduce4_f32(float& a, float& b, float& c, float& d) {
    if constexpr (G >= 4) {
        const bool hi1 = (threadIdx.x & (G / 2)) != 0;  // keeps (c, d), else (a, b)
        const bool hi2 = (threadIdx.x & (G / 4)) != 0;  // keeps the second of its two
        float x = (hi1 ? c : a) + __shfl_xor(hi1 ? a : c, G / 2, WAVE);
        float y = (hi1 ? d : b) + __shfl_xor(hi1 ? b : d, G / 2, WAVE);
        float keep = (hi2 ? y : x) + __shfl_xor(hi2 ? x : y, G / 4, WAVE);
#pragma unroll
        for (int off = G / 8; off > 0; off >>= 1) keep += __shfl_xor(keep, off, WAVE);
        const float other = __shfl_xor(keep, G / 4, WAVE);
        x = hi2 ? other : keep;
        y = hi2 ? keep : other;
        const float ox = __shfl_xor(x, G / 2, WAVE);
        const float oy = __shfl_xor(y, G / 2, WAVE);
        a = hi1 ? ox : x;
        b = hi1 ? oy : y;
        c = hi1 ? x : ox;
        d = hi1 ? y : oy;
    } else {
        group_allreduce2_f32<G>(a, b);
        group_allreduce2_f32<G>(c, d);
    }
}

template <typename T, int G, int KITER, class Link>  // K = KITER*G*VEC; KITER > 1 only at G = 64
__global__ __launch_bounds__(256) void k_glm_family_fvp(
    const T* __restrict__ X,            // [N][K] row-major
    const float* __restrict__ offset,   // [N] or NULL
    long long n_rows,
    const float* __restrict__ beta,     // [K]
    const float* __restrict__ v,        // [K], or NULL: diagonal mode
    LinkParams lp,
    float* __restrict__ slab            // [gridDim][K]
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
    const bool diag = v == nullptr;      // wave-uniform (grid-uniform)

    float xa[KITER][VEC];                // this lane's slice of step s
    float xb[KITER][VEC];                // ... and of step s+1
    float breg[KITER][VEC];              // this lane's beta slice (loop-invariant)
    float vreg[KITER][VEC];              // ... and its v slice (0 in diagonal mode)
    float acc[KITER][VEC];               // this lane's accumulator
#pragma unroll
    for (int c = 0; c < KITER; ++c)
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            breg[c][j] = beta[c * CHUNK + col0 + j];
            vreg[c][j] = diag ? 0.f : v[c * CHUNK + col0 + j];
            acc[c][j] = 0.f;
        }

    // Two steps per iteration, as in k_glm_family, where both steps' slices
    // and the three loop-invariant arrays fit (see "Registers" above).
    constexpr bool PAIRED = KITER * VEC < 32;
    const long long pair_stride = n_waves * 2;
    long long s = wave_id * 2;
    for (; PAIRED && (s + 2) * R <= n_rows; s += pair_stride) {
        const long long ra = s * R + grp;
        const long long rb = ra + R;
        const T* pa = X + ra * (long long)K + col0;
        const T* pb = pa + (long long)R * K;
#pragma unroll
        for (int c = 0; c < KITER; ++c) {
            // nontemporal: each X row is consumed once, from registers
            const u32x4_t va = __builtin_nontemporal_load((const u32x4_t*)(pa + c * CHUNK));
            const u32x4_t vb = __builtin_nontemporal_load((const u32x4_t*)(pb + c * CHUNK));
            TR::unpack(va, xa[c]);
            TR::unpack(vb, xb[c]);
        }
        float za = 0.f, zb = 0.f;
        if (offset) {  // wave-uniform
            za = __builtin_nontemporal_load(offset + ra);
            zb = __builtin_nontemporal_load(offset + rb);
        }
        float zap = 0.f, zbp = 0.f, ua = 0.f, ub = 0.f;
#pragma unroll
        for (int c = 0; c < KITER; ++c)
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                zap += xa[c][j] * breg[c][j];
                zbp += xb[c][j] * breg[c][j];
                ua += xa[c][j] * vreg[c][j];
                ub += xb[c][j] * vreg[c][j];
            }
        group_allreduce4_f32<G>(zap, zbp, ua, ub);
        za += zap;
        zb += zbp;
        float wa, wb;
        Link::weight(za, lp, wa);
        Link::weight(zb, lp, wb);
        if (diag) {
#pragma unroll
            for (int c = 0; c < KITER; ++c)
#pragma unroll
                for (int j = 0; j < VEC; ++j)
                    acc[c][j] += (wa * xa[c][j]) * xa[c][j] + (wb * xb[c][j]) * xb[c][j];
        } else {
            const float sa = wa * ua, sb = wb * ub;
#pragma unroll
            for (int c = 0; c < KITER; ++c)
#pragma unroll
                for (int j = 0; j < VEC; ++j)
                    acc[c][j] += sa * xa[c][j] + sb * xb[c][j];
        }
    }
    // One step at a time.  PAIRED: what is left of this wave's last pair, at
    // most two steps, of which the last may be ragged (one trip of the outer
    // loop).  Otherwise: every pair of this wave, with the same step-to-wave
    // assignment.
    for (; s * R < n_rows; s += pair_stride)
    for (int t = 0; t < 2; ++t) {
        const long long row = (s + t) * R + grp;
        if ((s + t) * R >= n_rows) break;  // wave-uniform
        const bool valid = row < n_rows;
        const T* pr = X + row * (long long)K + col0;
#pragma unroll
        for (int c = 0; c < KITER; ++c) {
            u32x4_t x4 = {0u, 0u, 0u, 0u};
            if (valid) x4 = __builtin_nontemporal_load((const u32x4_t*)(pr + c * CHUNK));
            TR::unpack(x4, xa[c]);
        }
        float z = 0.f;
        if (valid && offset) z = offset[row];
        float zp = 0.f, u = 0.f;
#pragma unroll
        for (int c = 0; c < KITER; ++c)
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                zp += xa[c][j] * breg[c][j];
                u += xa[c][j] * vreg[c][j];
            }
        group_allreduce2_f32<G>(zp, u);
        z += zp;
        float w;
        Link::weight(z, lp, w);
        if (!valid) w = 0.f;
        if (diag) {
#pragma unroll
            for (int c = 0; c < KITER; ++c)
#pragma unroll
                for (int j = 0; j < VEC; ++j) acc[c][j] += (w * xa[c][j]) * xa[c][j];
        } else {
            const float sw = w * u;
#pragma unroll
            for (int c = 0; c < KITER; ++c)
#pragma unroll
                for (int j = 0; j < VEC; ++j) acc[c][j] += sw * xa[c][j];
        }
    }

    // k_glm_family's block epilogue, kept as a copy: a shared helper changed
    // the ISA (see the note there).
    // lanes with equal lane % G hold partials of the same columns
#pragma unroll
    for (int c = 0; c < KITER; ++c)
#pragma unroll
        for (int j = 0; j < VEC; ++j)
#pragma unroll
            for (int off = WAVE / 2; off >= G; off >>= 1)
                acc[c][j] += __shfl_xor(acc[c][j], off, WAVE);

    // cross-wave reduction in LDS (dynamic: K floats), then one slab row
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* a_lds = reinterpret_cast<float*>(smem);  // [K]
    for (int w = 0; w < waves_per_block; ++w) {
        if (wid == w && lane < G) {
#pragma unroll
            for (int c = 0; c < KITER; ++c)
#pragma unroll
                for (int j = 0; j < VEC; ++j) {
                    const int col = c * CHUNK + col0 + j;
                    if (w == 0)
                        a_lds[col] = acc[c][j];
                    else
                        a_lds[col] += acc[c][j];
                }
        }
        __syncthreads();
    }
    float* slab_row = slab + (long long)blockIdx.x * K;
    for (int col = threadIdx.x; col < K; col += blockDim.x) slab_row[col] = a_lds[col];
}

extern "C" {

// out = fp64[K] = X^T (w * (X v)), or the diagonal sum_r w_r x_rk^2 when
// v_f32 is NULL; beta_f32 and v_f32 = fp32[K] device; offset_f32 (may be
// NULL) = fp32[n_rows] device; workspace holds the fp32 slab (ws_bytes >=
// grid*K*4; a smaller one shrinks the grid).  K as for fed_glm_family.
// Returns -2 bad dtype, -3 workspace too small, -4 unsupported K, -5 unknown
// link; every check precedes the first launch or write.
int fed_glm_family_fvp(
    const void* X, const float* offset_f32, long long n_rows, int K,
    const float* beta_f32, const float* v_f32, int link, double sigma,
    double* out, float* workspace, long long ws_bytes,
    int dtype, void* stream_v
) {
    hipStream_t stream = (hipStream_t)stream_v;
    // the launch plan of fed_glm_family, FED_GLM_GRID included
    RowGroupPlan plan;
    if (const int bad = plan_row_group(dtype, link, K, n_rows, ws_bytes, plan)) return bad;
    const int grid = plan.grid, block = plan.block;
    const int lds_bytes = (K * 4 + 15) & ~15;

    hipError_t err = hipMemsetAsync(out, 0, K * sizeof(double), stream);
    if (err != hipSuccess) return (int)err;

    const LinkParams lp = make_link_params(sigma);
    const int rc = dispatch_row_group(dtype, link, K, [&](auto t, auto l, auto g, auto kiter) {
        using T = typename decltype(t)::type;
        using Link = typename decltype(l)::type;
        hipLaunchKernelGGL((k_glm_family_fvp<T, decltype(g)::value, decltype(kiter)::value, Link>),
                           dim3(grid), dim3(block), lds_bytes, stream, (const T*)X, offset_f32,
                           n_rows, beta_f32, v_f32, lp, workspace);
    });
    if (rc != 0) return rc;
    hipError_t kerr = hipGetLastError();
    if (kerr != hipSuccess) return (int)kerr;

    return launch_colsum_reduce(workspace, grid, K, out, stream);
}

}  // extern "C"
