// Batched (16-column) GLM families on CDNA4 (gfx950) matrix cores:
// k_glm_family_batched and its C entry points fed_glm_family_batched, for the
// Poisson and Gaussian links of glm_links.hpp (16 chains), and
// fed_glm_softmax_batched, for the softmax GLM (16/CP chains of CP class
// slots).  Shared pieces and the overview of the GLM units are in
// fed_common.hpp; the fragment maps are the ones glm_logistic_batched.hip
// verifies with fed_mfma_probe.
//
//     Z[rows,16] = X[rows,K] . Theta[K,16] (+ offset[rows])   phase A, MFMA
//     term, resid = Stage::eval(y, z, column)                 per (row, column), f32
//     logp[b]   += term                                       fp64 from the thread outwards
//     G[K,16]   += X^T[K,rows] . R[rows,16]                   phase B, MFMA
//
// Split operands.  The logistic batched kernels round theta and the
// residual to one bf16 each; counts with exposure offsets and a Gaussian
// with a small sigma do not survive that (a gradient error of 10^4 units of
// 2^-24 * sum|row contribution| by operand rounding alone).  Three bf16
// pieces p0 = bf16(v), p1 = bf16(v - p0), p2 = bf16(v - p0 - p1) hold any
// finite f32 exactly, so theta arrives as bf16 [3][16][K] (transposed per
// piece) and phase A issues one MFMA per piece on the same X fragment, into
// one accumulator per piece, summed smallest piece first.  The residual is
// split the same way in the kernel into RP pieces (template parameter,
// default 3: exact) and phase B issues RP MFMAs per gathered X^T fragment.
//
// Middle stage (glm_links.hpp).  The kernel is a template over what a
// thread does with the z of its (row, column) slot; staging, phase A, phase
// B and the epilogue exist once.
//   ElementStage<Link>  the 16 columns are 16 independent chains; a slot is
//       evaluated on its own by Link::eval (Poisson, Gaussian).
//   SoftmaxStage        the 16 columns are 16/CP chains of CP class slots,
//       CP the next power of two >= C (2, 4, 8 or 16; a wave-uniform kernel
//       argument, not a template parameter: 8 instantiations instead of 32);
//       column g*CP + c is class c of chain g and y is the row's label.  A
//       padded class (c >= C) takes z = -inf, so its e and residual are 0
//       and its G column is exactly 0.  m = max and s = sum exp(z - m) over
//       the group are DPP butterflies (quad_perm x2, row_half_mirror,
//       row_mirror through __builtin_amdgcn_update_dpp; four steps, those
//       at or past CP masked): slot = tid + s*256 puts the 16 columns of a
//       row into the 16 adjacent lanes of one DPP row and every lane runs
//       the same SPT trips of the slot loop, so the cross-lane steps are
//       legal.
//       The lane c == y adds (z - m) - log(s) to its fp64 logp; out[0..16)
//       stay per-column sums and the host adds the CP columns of a chain.
//       Rows past n_rows are zero-filled, so their z are finite before the
//       mask (no NaN forms); |z| in the thousands stays finite.
//
// Geometry.  Block = 256 threads = 4 waves; a wave always works on 32 rows
// (two 16-row phase-A fragments, one 32-row phase-B reduction).
//   K >= 128: the 4 waves split K (QC = K/4 columns each) over ONE 32-row
//             tile; their partial Z meet in LDS.
//   K <  128: the 4 waves each take the whole K of their own 32 of the
//             tile's 128 rows; K = 8 and 16 zero-fill the fragment lanes
//             beyond K.
// Either way a wave's theta fragments (its K slice x 3 pieces) are loop
// invariant and live in registers for the whole kernel -- at K = 1024 three
// transposed theta images would be 96 KB of LDS -- and its G accumulators
// (QC/16 statically indexed f32x4 tiles) cover its own K slice over all of
// the block's tiles.  A narrow tile is small (2 KB at K = 8); there the
// small footprint lets up to 4 blocks share a CU, and that occupancy,
// not a deeper pipeline inside the block, is what keeps loads in flight.
//
// One tile: stage X (16-byte groups, four loads in flight per thread), y and
// offset (f32) into LDS | barrier | phase A from LDS, partial Z to LDS |
// barrier | one thread per (row, chain) slot: z, Stage::eval, fp64 logp,
// residual pieces to LDS (R^T image [piece][chain][row]) | barrier | phase
// B: X^T fragments by the u16 LDS gather of the v2 logistic kernel |
// barrier.  X is read from HBM exactly once.
//
// Ragged tiles.  Rows at or past n_rows are zero-filled by a conditional
// load (the clamped-address form spills, see TODO.md) and masked out of
// BOTH logp and the residual: exp(0) = 1 is not inert under the log link.
//
// Reductions.  Each (block, row-group) writes one fp32 slab row [K*16],
// reduced by the shared k_colsum_reduce.  logp: every thread owns one chain
// (thread & 15) and accumulates its terms in fp64; the block's per-chain
// sums are added with atomicAdd(double) into out[chain]; block 0 adds
// logp_const.
//
// Registers.  gfx950 ISA of all 24 instantiations (2 links and the softmax
// stage x 8 K, RP = 3) checked with
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -S --cuda-device-only \
//         -Rpass-analysis=kernel-resource-usage glm_family_batched.hip
// every one reports ScratchSize 0 and no VGPR/SGPR spill; the counts are in
// the tables at the dispatcher.  No inline assembly.
// Measurements: profiles/PROFILES.md "GLM family batched kernel" and
// "Softmax GLM".

#include "fed_common.hpp"
#include "glm_links.hpp"

#define FB_CH 16  // chains per call

typedef __attribute__((ext_vector_type(8))) __bf16 fb_bf16x8_t;
typedef __attribute__((ext_vector_type(4))) float fb_f32x4_t;
union fb_frag { fb_bf16x8_t v; unsigned short u[8]; U4 q; };

// fp32 -> bf16 bits, round to nearest even
__device__ __forceinline__ unsigned short fb_bf16_rne_bits(float f) {
    union { float f; unsigned int u; } cv;
    cv.f = f;
    const unsigned int rnd = 0x7fff + ((cv.u >> 16) & 1);
    return (unsigned short)((cv.u + rnd) >> 16);
}

template <int K>
struct FbGeom {
    static constexpr int WK = K >= 128 ? 4 : 1;          // waves splitting K
    static constexpr int WR = 4 / WK;                    // waves splitting rows
    static constexpr int TR = 32 * WR;                   // rows per tile
    static constexpr int QC = K / WK;                    // columns per wave
    static constexpr int NKS = QC >= 32 ? QC / 32 : 1;   // phase-A MFMA steps
    static constexpr int NT2 = QC >= 16 ? QC / 16 : 1;   // phase-B column tiles
    static constexpr int XS = K + 8;                     // X row stride (u16): +16 B
    static constexpr int RS = TR + 8;                    // R^T row stride (u16)
    static constexpr int SPT = TR * FB_CH / 256;         // (row, chain) slots per thread
    static constexpr int NG = TR * K / 8;                // 16-byte groups per tile
    // byte offsets into dynamic LDS, every one a multiple of 16
    static constexpr int X_BYTES = TR * XS * 2;
    static constexpr int ZC_BYTES = WK * TR * FB_CH * 4;
    static constexpr int Y_BYTES = TR * 4;
    static constexpr int RED_BYTES = 256 * 8;
    static constexpr int rt_bytes(int rp) { return rp * FB_CH * RS * 2; }
    static constexpr int lds_bytes(int rp) {
        return X_BYTES + rt_bytes(rp) + ZC_BYTES + 2 * Y_BYTES + RED_BYTES;
    }
    static_assert(X_BYTES % 16 == 0 && (FB_CH * RS * 2) % 16 == 0, "16-byte LDS sections");
};

template <class Stage, int K, int RP>
__global__ __launch_bounds__(256) void k_glm_family_batched(
    const unsigned short* __restrict__ X,        // [N][K] bf16 row-major
    const float* __restrict__ y,                 // [N]
    const float* __restrict__ offset,            // [N] or NULL
    long long n_rows,
    const unsigned short* __restrict__ theta_p,  // [3][16][K] bf16 pieces, transposed
    typename Stage::Params lp,
    double logp_const,
    double* __restrict__ logp_out,               // [16], pre-zeroed
    float* __restrict__ slab                     // [gridDim * WR][K*16]
) {
    using Gm = FbGeom<K>;
    constexpr int WK = Gm::WK, TR = Gm::TR, QC = Gm::QC, NKS = Gm::NKS, NT2 = Gm::NT2;
    constexpr int XS = Gm::XS, RS = Gm::RS;
    static_assert(RP >= 1 && RP <= 3, "1..3 residual pieces");
    const int lane = threadIdx.x & 63;
    const int wid = threadIdx.x >> 6;
    const int wk = wid % WK;          // this wave's K slice
    const int wr = wid / WK;          // this wave's 32-row group of the tile
    const int l15 = lane & 15;
    const int lq = lane >> 4;

    extern __shared__ __attribute__((aligned(16))) char smem[];
    unsigned short* x_lds = (unsigned short*)smem;                               // [TR][XS]
    unsigned short* rt_lds = (unsigned short*)(smem + Gm::X_BYTES);              // [RP][16][RS]
    float* zc_lds = (float*)(smem + Gm::X_BYTES + Gm::rt_bytes(RP));             // [WK][TR][16]
    float* y_lds = (float*)((char*)zc_lds + Gm::ZC_BYTES);                       // [TR]
    float* off_lds = y_lds + TR;                                                 // [TR]
    double* red_lds = (double*)(off_lds + TR);                                   // [256]

    // this wave's theta fragments: chain = lane & 15, 8 consecutive k
    fb_frag th[3][NKS];
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) {
            const int kloc = ks * 32 + lq * 8;
            th[p][ks].q = (U4){0, 0, 0, 0};
            if (QC % 32 == 0 || kloc < QC)
                th[p][ks].q =
                    *(const U4*)&theta_p[(long long)(p * FB_CH + l15) * K + wk * QC + kloc];
        }

    fb_f32x4_t g_acc[NT2];
#pragma unroll
    for (int t = 0; t < NT2; ++t) g_acc[t] = (fb_f32x4_t){0.f, 0.f, 0.f, 0.f};
    double logp_acc = 0.0;  // chain = threadIdx.x & 15

    const long long n_tiles = (n_rows + TR - 1) / TR;
    for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const long long row0 = tile * TR;

        // ---- stage the tile: four 16-byte loads in flight per thread ----
#pragma unroll
        for (int base = 0; base < Gm::NG; base += 1024) {
            U4 ld[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int g = base + u * 256 + (int)threadIdx.x;
                ld[u] = (U4){0, 0, 0, 0};
                if (Gm::NG % 1024 == 0 || g < Gm::NG) {
                    const long long row = row0 + g / (K / 8);
                    if (row < n_rows)
                        ld[u] = *(const U4*)&X[row * (long long)K + (g % (K / 8)) * 8];
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int g = base + u * 256 + (int)threadIdx.x;
                if (Gm::NG % 1024 == 0 || g < Gm::NG)
                    *(U4*)&x_lds[(g / (K / 8)) * XS + (g % (K / 8)) * 8] = ld[u];
            }
        }
        if (threadIdx.x < TR) {
            const long long r = row0 + threadIdx.x;
            float yv = 0.f, ov = 0.f;
            if (r < n_rows) {
                yv = y[r];
                if (offset) ov = offset[r];
            }
            y_lds[threadIdx.x] = yv;
            off_lds[threadIdx.x] = ov;
        }
        __syncthreads();

        // ---- phase A: this wave's partial Z of its 32 rows, per theta piece ----
        fb_f32x4_t za[3][2];
#pragma unroll
        for (int p = 0; p < 3; ++p)
            za[p][0] = za[p][1] = (fb_f32x4_t){0.f, 0.f, 0.f, 0.f};
        const int arow0 = wr * 32 + l15;
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) {
            const int kloc = ks * 32 + lq * 8;
            fb_frag a0, a1;
            a0.q = a1.q = (U4){0, 0, 0, 0};
            if (QC % 32 == 0 || kloc < QC) {
                a0.q = *(const U4*)&x_lds[arow0 * XS + wk * QC + kloc];
                a1.q = *(const U4*)&x_lds[(arow0 + 16) * XS + wk * QC + kloc];
            }
#pragma unroll
            for (int p = 0; p < 3; ++p) {
                za[p][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0.v, th[p][ks].v, za[p][0],
                                                                   0, 0, 0);
                za[p][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1.v, th[p][ks].v, za[p][1],
                                                                   0, 0, 0);
            }
        }
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = wr * 32 + h * 16 + lq * 4 + r;
                zc_lds[(wk * TR + row) * FB_CH + l15] = (za[2][h][r] + za[1][h][r]) + za[0][h][r];
            }
        __syncthreads();

        // ---- z, term, residual: one thread per (row, chain) slot ----
#pragma unroll
        for (int s = 0; s < Gm::SPT; ++s) {
            const int slot = (int)threadIdx.x + s * 256;
            const int row = slot >> 4;
            const int chain = slot & 15;
            float zs = zc_lds[row * FB_CH + chain];
#pragma unroll
            for (int w = 1; w < WK; ++w) zs += zc_lds[(w * TR + row) * FB_CH + chain];
            const float z = off_lds[row] + zs;
            float term, resid;
            Stage::eval(y_lds[row], z, chain, lp, term, resid);
            if (row0 + row >= n_rows) {
                term = 0.f;
                resid = 0.f;
            }
            logp_acc += (double)term;
            float rem = resid;
#pragma unroll
            for (int p = 0; p < RP; ++p) {
                const unsigned short bits = fb_bf16_rne_bits(rem);
                rt_lds[(p * FB_CH + chain) * RS + row] = bits;
                rem -= bf16_bits_to_f32(bits);
            }
        }
        __syncthreads();

        // ---- phase B: G[this wave's K slice] += X^T . R over its 32 rows ----
        fb_frag rb[RP];
#pragma unroll
        for (int p = 0; p < RP; ++p)
            rb[p].q = *(const U4*)&rt_lds[(p * FB_CH + l15) * RS + wr * 32 + lq * 8];
#pragma unroll
        for (int t2 = 0; t2 < NT2; ++t2) {
            fb_frag a;
            a.q = (U4){0, 0, 0, 0};
            if (QC % 16 == 0 || l15 < QC) {
                const unsigned short* col =
                    &x_lds[(wr * 32 + lq * 8) * XS + wk * QC + t2 * 16 + l15];
#pragma unroll
                for (int j = 0; j < 8; ++j) a.u[j] = col[j * XS];
            }
            fb_f32x4_t acc = g_acc[t2];
#pragma unroll
            for (int p = RP - 1; p >= 0; --p)
                acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.v, rb[p].v, acc, 0, 0, 0);
            g_acc[t2] = acc;
        }
        __syncthreads();  // x_lds, rt_lds and zc_lds are rewritten by the next tile
    }

    // ---- epilogue: one slab row per (block, row group); logp in fp64 ----
    float* slab_row = slab + ((long long)blockIdx.x * Gm::WR + wr) * ((long long)K * FB_CH);
#pragma unroll
    for (int t2 = 0; t2 < NT2; ++t2)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int kloc = t2 * 16 + lq * 4 + r;
            if (QC % 16 == 0 || kloc < QC)
                slab_row[(long long)(wk * QC + kloc) * FB_CH + l15] = g_acc[t2][r];
        }
    red_lds[threadIdx.x] = logp_acc;
    __syncthreads();
    if (threadIdx.x < FB_CH) {
        double s = blockIdx.x == 0 ? logp_const : 0.0;
        for (int i = threadIdx.x; i < 256; i += FB_CH) s += red_lds[i];
        atomicAdd(&logp_out[threadIdx.x], s);
    }
}

// Resource usage at RP = 3, from -Rpass-analysis=kernel-resource-usage
// (Poisson / Gaussian where they differ; occupancy in waves per SIMD, which
// with 4-wave blocks on 4 SIMDs is also blocks per CU; dynamic LDS per block):
//      K   VGPRs    AGPRs  occupancy  LDS bytes
//      8  114/98       8       4        28416
//     16     96        8       4        30464
//     32  103/108   12/16      4        34560
//     64  160/152     28       2        42752
//    128   75/74      16       5        23040
//    256  112/110     28       3        31232
//    512  192/188     52       2        47616
//   1024    218       88       1        80384
// All 16: ScratchSize 0, no SGPR or VGPR spill.  At K = 1024 the 96 theta
// and 64 G-accumulator registers leave one block per CU; a 2-waves-per-SIMD
// bound there spilled 144 bytes per lane and was dropped.
//
// The grid is sized to what is resident: 256 CUs x blocks per CU (K = 128
// is held to 4).
static int fb_blocks_per_cu(int K) {
    switch (K) {
        case 1024: return 1;
        case 512:  return 2;
        case 256:  return 3;
        case 64:   return 2;
        default:   return 4;
    }
}

// SoftmaxStage (8 more instantiations):
//      K   VGPRs    AGPRs  occupancy
//      8    117        8       4
//     16     99        8       4
//     32    106       12       4
//     64    155       28       2
//    128     77       16       5
//    256    123       28       3
//    512    141       52       2
//   1024    222       88       1
// All 8: ScratchSize 0, no SGPR or VGPR spill; LDS and occupancy as above,
// so both entry points size the grid by fb_blocks_per_cu.  (With the
// __shfl_xor butterfly the DPP one replaced, four more VGPRs each held the
// lane addresses, and K = 8 and 32 passed 128 registers: occupancy 3.)

template <class Stage, int K>
static void launch_fb(int grid, hipStream_t stream, const void* X, const float* y,
                      const float* offset, long long n_rows, const void* theta_p,
                      typename Stage::Params lp, double logp_const, double* out,
                      float* workspace) {
    constexpr int RP = 3;
    hipLaunchKernelGGL((k_glm_family_batched<Stage, K, RP>), dim3(grid), dim3(256),
                       FbGeom<K>::lds_bytes(RP), stream, (const unsigned short*)X, y, offset,
                       n_rows, (const unsigned short*)theta_p, lp, logp_const, out, workspace);
}

template <class Stage, typename... Args>
static bool dispatch_fb(int K, Args... args) {
    switch (K) {
        case 8:    launch_fb<Stage, 8>(args...); return true;
        case 16:   launch_fb<Stage, 16>(args...); return true;
        case 32:   launch_fb<Stage, 32>(args...); return true;
        case 64:   launch_fb<Stage, 64>(args...); return true;
        case 128:  launch_fb<Stage, 128>(args...); return true;
        case 256:  launch_fb<Stage, 256>(args...); return true;
        case 512:  launch_fb<Stage, 512>(args...); return true;
        case 1024: launch_fb<Stage, 1024>(args...); return true;
        default:   return false;
    }
}

static bool fb_supported_k(int K) { return K >= 8 && K <= 1024 && (K & (K - 1)) == 0; }

// What the entry points share once their arguments are checked: the grid,
// the zeroed out, the kernel and the slab reduction.  -3 workspace too small.
template <class Stage>
static int fb_run(const void* X, const float* y, const float* offset, long long n_rows, int K,
                  const void* theta_p, typename Stage::Params lp, double logp_const, double* out,
                  float* workspace, long long ws_bytes, int blocks_per_cu, hipStream_t stream) {
    const int row_groups = K >= 128 ? 1 : 4;   // FbGeom<K>::WR
    const int tile_rows = 32 * row_groups;     // FbGeom<K>::TR

    const long long n_tiles = (n_rows + tile_rows - 1) / tile_rows;
    int grid = 256 * blocks_per_cu;
    if (n_tiles < grid) grid = n_tiles < 1 ? 1 : (int)n_tiles;
    // FED_GLM_BATCHED_GRID caps the grid (tests reach several tiles per
    // block at small N with it); read per call
    if (const char* ge = getenv("FED_GLM_BATCHED_GRID")) {
        const int v = atoi(ge);
        if (v >= 1 && v < grid) grid = v;
    }
    const long long block_bytes = (long long)row_groups * K * FB_CH * sizeof(float);
    if ((long long)grid * block_bytes > ws_bytes) grid = (int)(ws_bytes / block_bytes);
    if (grid < 1) return -3;

    const long long out_cols = FB_CH + (long long)K * FB_CH;
    hipError_t err = hipMemsetAsync(out, 0, out_cols * sizeof(double), stream);
    if (err != hipSuccess) return (int)err;

    if (!dispatch_fb<Stage>(K, grid, stream, X, y, offset, n_rows, theta_p, lp, logp_const, out,
                            workspace))
        return -4;
    hipError_t kerr = hipGetLastError();
    if (kerr != hipSuccess) return (int)kerr;

    return launch_colsum_reduce(workspace, grid * row_groups, K * FB_CH, out + FB_CH, stream);
}

extern "C" {

// out = fp64[16 + K*16] = [logp[16] | G[K][16]] (the layout of
// fed_logistic_glm_batched); X = bf16[n_rows][K]; y_f32 and offset_f32 (may
// be NULL) = fp32[n_rows]; theta_pieces_bf16 = bf16[3][16][K], the three
// split pieces of theta, each transposed; workspace holds the fp32 slab
// (ws_bytes >= rows_groups * K*16*4 for at least one block).  K in {8, 16,
// ..., 1024}; link is FED_LINK_POISSON or FED_LINK_GAUSSIAN.  Returns -3
// workspace too small, -4 unsupported K, -5 unknown link; all of them
// before anything is launched.
int fed_glm_family_batched(
    const void* X, const float* y_f32, const float* offset_f32,
    long long n_rows, int K, const void* theta_pieces_bf16, int link,
    double sigma, double logp_const,
    double* out, float* workspace, long long ws_bytes,
    void* stream_v
) {
    hipStream_t stream = (hipStream_t)stream_v;
    if (link != FED_LINK_POISSON && link != FED_LINK_GAUSSIAN) return -5;
    if (!fb_supported_k(K)) return -4;
    const LinkParams lp = make_link_params(sigma);
    if (link == FED_LINK_POISSON)
        return fb_run<ElementStage<PoissonLink>>(X, y_f32, offset_f32, n_rows, K,
                                                 theta_pieces_bf16, lp, logp_const, out,
                                                 workspace, ws_bytes, fb_blocks_per_cu(K), stream);
    return fb_run<ElementStage<GaussianLink>>(X, y_f32, offset_f32, n_rows, K, theta_pieces_bf16,
                                              lp, logp_const, out, workspace, ws_bytes,
                                              fb_blocks_per_cu(K), stream);
}

// Softmax (multinomial) GLM on the same kernel with the row-coupled
// SoftmaxStage: the 16 columns are 16/CP chains of CP class slots, CP the
// next power of two >= n_classes.  y_f32 = fp32[n_rows] holds the labels in
// [0, n_classes) (exact in f32); theta_pieces_bf16 = bf16[3][16][K] with
// column g*CP + c the class c of chain g (what the columns of padded
// classes hold is not read into any result).  out, workspace and the grid
// as in fed_glm_family_batched: out[0..16) are per-column sums, the logp of
// chain g is the sum of out[g*CP .. g*CP+CP), and the G columns of padded
// classes are exactly 0.  Returns -3 workspace too small, -4 unsupported K,
// -6 n_classes outside [2, 16]; all of them before anything is launched.
int fed_glm_softmax_batched(
    const void* X, const float* y_f32, long long n_rows, int K,
    const void* theta_pieces_bf16, int n_classes,
    double* out, float* workspace, long long ws_bytes,
    void* stream_v
) {
    hipStream_t stream = (hipStream_t)stream_v;
    if (!fb_supported_k(K)) return -4;
    if (n_classes < 2 || n_classes > FB_CH) return -6;
    SoftmaxParams sp;
    sp.n_classes = n_classes;
    sp.cp = 2;
    while (sp.cp < n_classes) sp.cp *= 2;
    return fb_run<SoftmaxStage>(X, y_f32, nullptr, n_rows, K, theta_pieces_bf16, sp, 0.0, out,
                                workspace, ws_bytes, fb_blocks_per_cu(K), stream);
}

}  // extern "C"
