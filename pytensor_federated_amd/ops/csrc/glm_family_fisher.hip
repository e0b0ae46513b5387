// Fisher information of the Poisson and Gaussian GLM families on CDNA4
// (gfx950) matrix cores: k_glm_fisher and its C entry point
// fed_glm_family_fisher.  Shared pieces are in fed_common.hpp, the link
// policies (Link::weight) in glm_links.hpp; the MFMA fragment maps are the
// ones glm_logistic_batched.hip verifies with fed_mfma_probe.
//
//     z[rows]  = X[rows,K] . beta[K] (+ offset[rows])     f32 VALU, beta not rounded
//     w[rows]  = Link::weight(z) = -d^2 term / dz^2        Poisson exp(z), Gaussian 1/sigma^2
//     H[K,K]  += X^T[K,rows] . (w (.) X)[rows,K]            bf16 MFMA 16x16x32, f32 accumulators
//
// Both links are canonical, so H is the expected and the observed
// information, -d^2 logp / d beta^2.  y is not an input.
//
// Split operand.  The A operand is X^T, whose bf16 values are used as they
// are.  The B operand v = f32(w * x) is split on the device into RP bf16
// pieces p0 = bf16(v), p1 = bf16(v - p0), p2 = bf16(v - p0 - p1) (template
// parameter, default 3: any finite f32 exactly; bf16() rounds to nearest
// even, by the packed hardware conversion) and each output tile issues one
// MFMA per piece on the same A fragment, smallest piece first.
//
// Panels.  H is cut into panels of PW = min(K, 128) columns; a block owns
// one panel pair (I, J) with I <= J and a strided set of row tiles, so the
// grid is (panel pair) x (row chunk) with the pair running fastest: the
// blocks that read the same row tiles are neighbours in the launch order
// and run at about the same time.  Only pairs of the upper triangle are
// computed, and inside a diagonal pair the wave that would hold the strictly
// lower quarter is idle; the reduce kernel takes H[i][j] for i <= j and
// writes it to (i, j) and (j, i), so the output is symmetric bit for bit.
//
// Geometry.  Block = 256 threads = 4 waves; a row tile is TR rows (64 at
// K >= 128, 128 at K = 64, 256 below).
//   K >= 32: the 4 waves form a 2 x 2 grid over the PW x PW pair, each with
//            (PW/32)^2 accumulator tiles (16 tiles = 64 f32 registers at
//            PW = 128), over all rows of the tile.
//   K <  32: one 16 x 16 tile (K = 8 zero-fills columns 8..15 of the LDS
//            images once); the 4 waves split the tile's 32-row MFMA steps
//            and each writes a slab row of its own.
// Staging.  A thread owns an 8 row x 4 column unit of panel I and, off the
// diagonal, the same unit of panel J: 8 (16) 8-byte loads in flight, rows at
// or past n_rows zero-filled by a conditional load; the loads of the next
// tile are issued before this tile's MFMAs.  All 256 threads stage (with
// 8 x 8 units half of the waves carried the whole split and the kernel ran
// at the pace of their SIMDs).  The unit is transposed in registers and
// written with 16-byte stores into the transposed LDS images xt[col][slot]
// (A) and wx[piece][col][slot] (B), so every MFMA fragment is one 16-byte LDS
// read along the reduction index.  A unit's rows are TR/8 apart in the
// tile (a wave's load then reads contiguous memory) and land in 8
// consecutive slots; both images and w use the same slot order, which the
// sum over rows does not see.  The 16-byte chunks of an image row are
// XOR-swizzled by the column quad: conflict-free ds_write_b128 groups, 2-way
// fragment reads.
//
// z and w.  K <= 128 (one panel pair): the block forms z itself -- each unit
// adds its 4-column partial dot per row (f32 beta in registers), four
// neighbouring lanes add theirs by shuffles, the partials meet in LDS, one
// thread per row adds them in a fixed order, applies Link::weight and
// forces w = 0 for rows at or past n_rows (exp(0) = 1 is not inert).  X is
// read from HBM exactly once.  K > 128: a block sees two panels of a row
// only, so k_fisher_weights forms w[n_rows] in one pass over X (32 lanes
// per row) into the head of the workspace and the panel blocks read w from
// there.
//
// Traffic, as a multiple of the shard size: a pair reads its two panels (one
// on the diagonal) of every row tile, which over the NP(NP+1)/2 pairs is NP
// panels per column, NP = K/128, plus the weights pass:
//      K <= 128   1x   (HBM)
//      K  = 256   3x   (1 weights pass + 2; re-reads served by L2 / Infinity Cache
//      K  = 512   5x    when the neighbouring blocks keep pace, HBM otherwise)
//      K  = 1024  9x
//
// Reduction.  Each (block, row-split wave) writes one fp32 slab row
// [PW*PW]; k_fisher_reduce sums the rows of a pair in fp64 in a fixed order
// (no atomics) and mirrors.  Every entry of out is written; nothing is
// pre-zeroed.
//
// Registers.  gfx950 ISA of all 16 instantiations (2 links x 8 K, RP = 3)
// and of the 6 weights kernels checked with
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -S --cuda-device-only \
//         -Rpass-analysis=kernel-resource-usage glm_family_fisher.hip
// every one reports ScratchSize 0 and no VGPR/SGPR spill; the counts are in
// the table at the dispatcher.  No inline assembly.
// Measurements: profiles/PROFILES.md "GLM Fisher kernel".

#include "fed_common.hpp"
#include "glm_links.hpp"

typedef __attribute__((ext_vector_type(8))) __bf16 fs_bf16x8_t;
typedef __attribute__((ext_vector_type(4))) float fs_f32x4_t;
typedef __attribute__((ext_vector_type(8))) float fs_f32x8_t;
union fs_frag { fs_bf16x8_t v; unsigned short u[8]; U4 q; };
struct U2 { unsigned int x, y; };
union fs_half { unsigned short u[4]; U2 q; };

template <int K>
struct FsGeom {
    static constexpr int PW = K < 128 ? K : 128;          // panel width
    static constexpr int PWL = PW < 16 ? 16 : PW;         // LDS image columns
    static constexpr int NP = K / PW;                     // panels
    static constexpr int NPP = NP * (NP + 1) / 2;         // panel pairs, I <= J
    static constexpr bool FUSED = NP == 1;                // z formed in the block
    static constexpr int TR = K >= 128 ? 64 : (K == 64 ? 128 : 256);  // rows per tile
    static constexpr int NT = PWL / 16;                   // 16-column tiles per side
    static constexpr int WT = NT >= 2 ? 2 : 1;            // waves per side
    static constexpr int WRS = 4 / (WT * WT);             // waves splitting the rows
    static constexpr int TI = NT / WT;                    // tiles per wave per side
    static constexpr int KS = TR / 32;                    // 32-row MFMA steps per tile
    static constexpr int RS = TR + 8;                     // image row stride (u16): +16 B
    static constexpr int CB4 = PW / 4;                    // 4-column quads per panel row
    static constexpr int RBN = TR / 8;                    // 8-slot groups per tile
    static constexpr int UNITS = CB4 * RBN;               // 8x4 units per panel tile
    static constexpr int SH = CB4 < 4 ? CB4 : 4;          // lanes adding their z partials
    static constexpr int ZPW = CB4 / SH;                  // z partials per row in LDS
    // byte offsets into dynamic LDS, every one a multiple of 16
    static constexpr int IMG_BYTES = PWL * RS * 2;
    static constexpr int ZP_BYTES = FUSED ? TR * ZPW * 4 : 0;
    static constexpr int W_BYTES = TR * 4;
    static constexpr int lds_bytes(int rp) { return (1 + rp) * IMG_BYTES + ZP_BYTES + W_BYTES; }
    static_assert(IMG_BYTES % 16 == 0 && (RS * 2) % 16 == 0, "16-byte LDS sections");
    static_assert(UNITS <= 256, "one unit per thread");
    static_assert(RBN >= 8, "the chunk swizzle stays inside an image row");
    static_assert(TR <= 256, "one thread per row");
};

template <class Link, int K, int RP>
__global__ __launch_bounds__(256, 2) void k_glm_fisher(
    const unsigned short* __restrict__ X,   // [N][K] bf16 row-major
    const float* __restrict__ offset,       // [N] or NULL (K <= 128 only)
    long long n_rows,
    const float* __restrict__ beta,         // [K] f32 (K <= 128 only)
    const float* __restrict__ w_in,         // [N] f32 weights (K > 128 only)
    LinkParams lp,
    float* __restrict__ slab                // [gridDim * WRS][PW*PW]
) {
    using Gm = FsGeom<K>;
    constexpr int PW = Gm::PW, PWL = Gm::PWL, NP = Gm::NP, NPP = Gm::NPP, TR = Gm::TR;
    constexpr int WT = Gm::WT, WRS = Gm::WRS, TI = Gm::TI, KS = Gm::KS, RS = Gm::RS;
    constexpr int CB4 = Gm::CB4, RBN = Gm::RBN, SH = Gm::SH, ZPW = Gm::ZPW;
    static_assert(RP >= 1 && RP <= 3, "1..3 pieces of w*x");
    const int lane = threadIdx.x & 63;
    const int wid = threadIdx.x >> 6;
    const int wi = WT == 2 ? wid >> 1 : 0;   // this wave's tile rows of the pair
    const int wj = WT == 2 ? wid & 1 : 0;    // this wave's tile columns of the pair
    const int wr = WT == 2 ? 0 : wid;        // this wave's share of the MFMA steps
    const int l15 = lane & 15;
    const int lq = lane >> 4;

    extern __shared__ __attribute__((aligned(16))) char smem[];
    unsigned short* xt_lds = (unsigned short*)smem;                          // [PWL][RS]
    unsigned short* wx_lds = (unsigned short*)(smem + Gm::IMG_BYTES);        // [RP][PWL][RS]
    float* zp_lds = (float*)(smem + (1 + RP) * Gm::IMG_BYTES);               // [TR][ZPW]
    float* w_lds = (float*)(smem + (1 + RP) * Gm::IMG_BYTES + Gm::ZP_BYTES); // [TR]

    // this block's panel pair (I <= J) and row chunk; the pair runs fastest
    const int pair = (int)(blockIdx.x % NPP);
    const int chunk = (int)(blockIdx.x / NPP);
    const int n_chunks = (int)(gridDim.x / NPP);
    int pI = 0, pJ = 0;
    {
        int rest = pair;
        while (rest >= NP - pI) {
            rest -= NP - pI;
            ++pI;
        }
        pJ = pI + rest;
    }
    const bool diag = pI == pJ;

    // this thread's unit: 8 rows x 4 columns of panel I (A image) and, off
    // the diagonal, the same unit of panel J (B images).  The column quad
    // runs fastest over the lanes and the unit's rows are RBN apart, so a
    // wave's load instruction reads contiguous memory; the unit's 8 rows go
    // to image slots rb*8 .. rb*8+7.  The reduction runs over the slots, and
    // xt, wx and w_lds all use the same slot order, so H does not see it.
    const int uu = (int)threadIdx.x;
    const bool active = uu < Gm::UNITS;
    const int cb4 = uu % CB4;
    const int rb = uu / CB4;
    const int colA = pI * PW + cb4 * 4;
    const int colB = pJ * PW + cb4 * 4;
    // 16-byte chunk rb of an image row is stored at chunk rb ^ swz(column
    // quad): the 8 lanes of a ds_write_b128 group (8 column quads, one rb)
    // then hit 8 different bank quads, and the MFMA fragment reads stay 2-way
    const int chunk_w = rb ^ (cb4 & 7);

    float bt[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) bt[c] = 0.f;
    if (Gm::FUSED && active) {
#pragma unroll
        for (int c = 0; c < 4; ++c) bt[c] = beta[colA + c];
    }

    if (PW < PWL) {  // K = 8: image columns 8..15 stay zero for the whole kernel
        for (int i = threadIdx.x; i < (1 + RP) * PWL * RS; i += 256) xt_lds[i] = 0;
        __syncthreads();
    }

    fs_f32x4_t acc[TI][TI];
#pragma unroll
    for (int a = 0; a < TI; ++a)
#pragma unroll
        for (int b = 0; b < TI; ++b) acc[a][b] = (fs_f32x4_t){0.f, 0.f, 0.f, 0.f};

    // the row of the tile at row0 that image slot s holds
    auto slot_row = [&](long long row0, int s) { return row0 + (s & 7) * RBN + (s >> 3); };

    // this thread's units of a tile: 8 (16 off the diagonal) 8-byte loads in
    // flight (and, for K > 128, the weight of slot threadIdx.x); rows at or
    // past n_rows are 0
    auto load_unit = [&](long long tile, fs_half (&ua)[8], fs_half (&ub)[8], float& wv) {
        const long long row0 = tile * TR;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            ua[j].q = (U2){0, 0};
            ub[j].q = (U2){0, 0};
            const long long row = row0 + j * RBN + rb;
            if (active && row < n_rows) {
                ua[j].q = *(const U2*)&X[row * (long long)K + colA];
                if (NP > 1 && !diag) ub[j].q = *(const U2*)&X[row * (long long)K + colB];
            }
        }
        wv = 0.f;
        if (!Gm::FUSED && threadIdx.x < TR) {
            const long long r = slot_row(row0, (int)threadIdx.x);
            if (r < n_rows) wv = w_in[r];
        }
    };

    const long long n_tiles = (n_rows + TR - 1) / TR;
    fs_half lda[8], ldb[8];
    float w_row = 0.f;
    if (chunk < n_tiles) load_unit(chunk, lda, ldb, w_row);
    for (long long tile = chunk; tile < n_tiles; tile += n_chunks) {
        const long long row0 = tile * TR;

        // ---- w of the tile's slots into w_lds ----
        if (Gm::FUSED) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                float zp = 0.f;
#pragma unroll
                for (int c = 0; c < 4; ++c) zp += bf16_bits_to_f32(lda[j].u[c]) * bt[c];
                // the SH lanes of a row's neighbouring column quads
                if (SH >= 2) zp += __shfl_xor(zp, 1, WAVE);
                if (SH >= 4) zp += __shfl_xor(zp, 2, WAVE);
                if (active && cb4 % SH == 0) zp_lds[(rb * 8 + j) * ZPW + cb4 / SH] = zp;
            }
            __syncthreads();
            if (threadIdx.x < TR) {
                const long long r = slot_row(row0, (int)threadIdx.x);
                float z = 0.f;
#pragma unroll
                for (int c = 0; c < ZPW; ++c) z += zp_lds[threadIdx.x * ZPW + c];
                float w = 0.f;
                if (r < n_rows) {
                    if (offset) z += offset[r];
                    Link::weight(z, lp, w);
                }
                w_lds[threadIdx.x] = w;
            }
        } else {
            if (threadIdx.x < TR) w_lds[threadIdx.x] = w_row;
        }
        __syncthreads();

        // ---- transposed images: xt[col][slot], wx[piece][col][slot] ----
        if (active) {
            fs_f32x8_t wv;
#pragma unroll
            for (int j = 0; j < 8; ++j) wv[j] = w_lds[rb * 8 + j];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int at = (cb4 * 4 + c) * RS + chunk_w * 8;
                fs_frag t;
#pragma unroll
                for (int j = 0; j < 8; ++j) t.u[j] = lda[j].u[c];
                *(U4*)&xt_lds[at] = t.q;
                if (NP > 1 && !diag) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) t.u[j] = ldb[j].u[c];
                }
                // vector conversions: packed round-to-nearest-even converts
                fs_f32x8_t rem = wv * __builtin_convertvector(t.v, fs_f32x8_t);
#pragma unroll
                for (int p = 0; p < RP; ++p) {
                    t.v = __builtin_convertvector(rem, fs_bf16x8_t);
                    rem -= __builtin_convertvector(t.v, fs_f32x8_t);
                    *(U4*)&wx_lds[p * PWL * RS + at] = t.q;
                }
            }
        }
        __syncthreads();

        // ---- the next tile's loads fly under this tile's MFMAs ----
        if (tile + n_chunks < n_tiles) load_unit(tile + n_chunks, lda, ldb, w_row);

        // ---- H[pair] += X_I^T . (w X_J) over the tile's slots ----
        if (!(WT == 2 && diag && wi > wj)) {
#pragma unroll
            for (int ks = 0; ks < KS / WRS; ++ks) {
                const int q = (ks * WRS + wr) * 4 + lq;  // 16-byte chunk of the image row
                fs_frag a[TI];
#pragma unroll
                for (int ti = 0; ti < TI; ++ti) {
                    const int col = (wi * TI + ti) * 16 + l15;
                    a[ti].q = *(const U4*)&xt_lds[col * RS + (q ^ ((col >> 2) & 7)) * 8];
                }
#pragma unroll
                for (int tj = 0; tj < TI; ++tj) {
                    const int col = (wj * TI + tj) * 16 + l15;
                    const int at = col * RS + (q ^ ((col >> 2) & 7)) * 8;
                    fs_frag b[RP];
#pragma unroll
                    for (int p = 0; p < RP; ++p) b[p].q = *(const U4*)&wx_lds[p * PWL * RS + at];
#pragma unroll
                    for (int ti = 0; ti < TI; ++ti) {
                        fs_f32x4_t c = acc[ti][tj];
#pragma unroll
                        for (int p = RP - 1; p >= 0; --p)
                            c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[ti].v, b[p].v, c, 0, 0,
                                                                        0);
                        acc[ti][tj] = c;
                    }
                }
            }
        }
        __syncthreads();  // the images, zp_lds and w_lds are rewritten by the next tile
    }

    // ---- epilogue: one slab row per (block, row-split wave) ----
    float* slab_row = slab + ((long long)blockIdx.x * WRS + wr) * (long long)(PW * PW);
#pragma unroll
    for (int ti = 0; ti < TI; ++ti)
#pragma unroll
        for (int tj = 0; tj < TI; ++tj)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = (wi * TI + ti) * 16 + lq * 4 + r;
                const int j = (wj * TI + tj) * 16 + l15;
                if (PW == PWL || (i < PW && j < PW)) slab_row[i * PW + j] = acc[ti][tj][r];
            }
}

// w[r] = Link::weight(x_r . beta (+ offset[r])) for K > 128: 32 lanes per
// row, K/256 16-byte vectors per lane, f32 beta in registers.
template <class Link, int K>
__global__ __launch_bounds__(256) void k_fisher_weights(
    const unsigned short* __restrict__ X, const float* __restrict__ offset, long long n_rows,
    const float* __restrict__ beta, LinkParams lp, float* __restrict__ w_out) {
    constexpr int NV = K / 256;
    static_assert(K % 256 == 0, "32 lanes x 8 columns");
    const int l31 = threadIdx.x & 31;
    float bt[NV][8];
#pragma unroll
    for (int m = 0; m < NV; ++m)
#pragma unroll
        for (int c = 0; c < 8; ++c) bt[m][c] = beta[(m * 32 + l31) * 8 + c];
    const long long groups = (long long)gridDim.x * 8;
    for (long long r = (long long)blockIdx.x * 8 + (threadIdx.x >> 5); r < n_rows; r += groups) {
        fs_frag ld[NV];
#pragma unroll
        for (int m = 0; m < NV; ++m) ld[m].q = *(const U4*)&X[r * (long long)K + (m * 32 + l31) * 8];
        float z = 0.f;
#pragma unroll
        for (int m = 0; m < NV; ++m)
#pragma unroll
            for (int c = 0; c < 8; ++c) z += bf16_bits_to_f32(ld[m].u[c]) * bt[m][c];
#pragma unroll
        for (int off = 16; off > 0; off >>= 1) z += __shfl_xor(z, off, WAVE);
        if (l31 == 0) {
            if (offset) z += offset[r];
            float w;
            Link::weight(z, lp, w);
            w_out[r] = w;
        }
    }
}

// out[K][K] (fp64, full symmetric) from the slab: block = (256 / SL) entries
// x SL slices of the slab rows; a slice's partial sums meet in LDS and are
// added in slice order, so the sum has one fixed order.  The entry (i, j) of
// pair (I, J) goes to out[I*PW+i][J*PW+j] and to its mirror; on a diagonal
// pair only i <= j is taken.
__global__ __launch_bounds__(256) void k_fisher_reduce(
    const float* __restrict__ slab, int n_slab_rows /* per pair */, int wrs, int NP, int PW, int K,
    int SL, double* __restrict__ out) {
    __shared__ double red[256];
    const int E = 256 / SL;
    const int NPP = NP * (NP + 1) / 2;
    const int pw2 = PW * PW;
    const int el = threadIdx.x % E;
    const int s = threadIdx.x / E;
    const long long ge = (long long)blockIdx.x * E + el;
    const int pair = (int)(ge / pw2);
    const int e = (int)(ge % pw2);
    double sum = 0.0;
    if (pair < NPP) {
        for (int q = s; q < n_slab_rows; q += SL) {
            const long long row = ((long long)(q / wrs) * NPP + pair) * wrs + q % wrs;
            sum += (double)slab[row * pw2 + e];
        }
    }
    red[threadIdx.x] = sum;
    __syncthreads();
    if (s != 0 || pair >= NPP) return;
    double total = 0.0;
    for (int t = 0; t < SL; ++t) total += red[t * E + el];
    int pI = 0, rest = pair;
    while (rest >= NP - pI) {
        rest -= NP - pI;
        ++pI;
    }
    const int pJ = pI + rest;
    const int i = e / PW, j = e % PW;
    if (pI == pJ && i > j) return;
    const long long gi = (long long)pI * PW + i, gj = (long long)pJ * PW + j;
    out[gi * K + gj] = total;
    out[gj * K + gi] = total;
}

// Resource usage at RP = 3, from -Rpass-analysis=kernel-resource-usage
// (Poisson / Gaussian where they differ; occupancy in waves per SIMD, which
// with 4-wave blocks on 4 SIMDs is also the register bound on blocks per CU;
// dynamic LDS per block):
//      K   VGPRs    AGPRs  occupancy  LDS bytes   (k_glm_fisher, __launch_bounds__(256, 2))
//      8   94/84       0       5        35840
//     16   94/85       0       5        35840
//     32    112        0       4        70656
//     64    122        0       4        72192
//    128    168        0       3        76032
//    256    157        0       3        73984
//    512    157        0       3        73984
//   1024    157        0       3        73984
// k_fisher_weights (K = 256, 512, 1024): 27, 43, 72 VGPRs for Poisson, 6 for
// Gaussian (w is a constant; the loads of X are dropped), no AGPRs, no LDS;
// k_fisher_reduce: 24 VGPRs, 2048 bytes of static LDS.
// All of them: ScratchSize 0, no SGPR or VGPR spill.
//
// The grid is sized to what is resident: 256 CUs x blocks per CU, which LDS
// (160 KB per CU) holds to two from K = 32 up and to four below.
static int fs_blocks_per_cu(int K) { return K >= 32 ? 2 : 4; }

template <class Link, int K>
static void launch_fs(int grid, int wgrid, hipStream_t stream, const void* X, const float* offset,
                      long long n_rows, const float* beta, LinkParams lp, float* w_buf,
                      float* slab) {
    constexpr int RP = 3;
    if constexpr (!FsGeom<K>::FUSED)
        hipLaunchKernelGGL((k_fisher_weights<Link, K>), dim3(wgrid), dim3(256), 0, stream,
                           (const unsigned short*)X, offset, n_rows, beta, lp, w_buf);
    hipLaunchKernelGGL((k_glm_fisher<Link, K, RP>), dim3(grid), dim3(256),
                       FsGeom<K>::lds_bytes(RP), stream, (const unsigned short*)X, offset, n_rows,
                       beta, w_buf, lp, slab);
}

template <class Link, typename... Args>
static bool dispatch_fs(int K, Args... args) {
    switch (K) {
        case 8:    launch_fs<Link, 8>(args...); return true;
        case 16:   launch_fs<Link, 16>(args...); return true;
        case 32:   launch_fs<Link, 32>(args...); return true;
        case 64:   launch_fs<Link, 64>(args...); return true;
        case 128:  launch_fs<Link, 128>(args...); return true;
        case 256:  launch_fs<Link, 256>(args...); return true;
        case 512:  launch_fs<Link, 512>(args...); return true;
        case 1024: launch_fs<Link, 1024>(args...); return true;
        default:   return false;
    }
}

extern "C" {

// Rows per tile of the kernel at K (FsGeom<K>::TR), 0 for an unsupported K;
// the edge-shape tests take their row counts from it.
int fed_glm_family_fisher_tile_rows(int K) {
    if (K < 8 || K > 1024 || (K & (K - 1)) != 0) return 0;
    return K >= 128 ? 64 : (K == 64 ? 128 : 256);
}

// out = fp64[K*K], row-major, full symmetric: H = X^T diag(w) X with
// w = Link::weight(X.beta (+ offset)); X = bf16[n_rows][K]; offset_f32 (may
// be NULL) = fp32[n_rows]; beta_f32 = fp32[K].  The workspace holds, for
// K > 128, n_rows f32 weights (rounded up to 16 bytes) and then the fp32
// slab: one row of min(K,128)^2 floats per block (four per block at K < 32);
// the grid is sized to it.  K in {8, 16, ..., 1024}; link is
// FED_LINK_POISSON or FED_LINK_GAUSSIAN.  Returns -3 workspace too small,
// -4 unsupported K, -5 unknown link; all of them before anything is
// launched.
int fed_glm_family_fisher(
    const void* X, const float* offset_f32, long long n_rows, int K,
    const float* beta_f32, int link, double sigma,
    double* out, float* workspace, long long ws_bytes, void* stream_v
) {
    hipStream_t stream = (hipStream_t)stream_v;
    if (link != FED_LINK_POISSON && link != FED_LINK_GAUSSIAN) return -5;
    const int tile_rows = fed_glm_family_fisher_tile_rows(K);
    if (tile_rows == 0) return -4;
    if (n_rows < 0) n_rows = 0;
    const int PW = K < 128 ? K : 128;
    const int NP = K / PW;
    const int NPP = NP * (NP + 1) / 2;
    const int wrs = K < 32 ? 4 : 1;  // FsGeom<K>::WRS

    // K > 128: the weights take the head of the workspace
    const long long w_bytes = NP > 1 ? ((n_rows + 3) / 4) * 16 : 0;
    if (ws_bytes < w_bytes) return -3;
    float* slab = workspace + w_bytes / 4;
    const long long slab_bytes = ws_bytes - w_bytes;

    const long long n_tiles = (n_rows + tile_rows - 1) / tile_rows;
    long long chunks = 256 * fs_blocks_per_cu(K) / NPP;  // what is resident
    if (n_tiles < chunks) chunks = n_tiles < 1 ? 1 : n_tiles;
    // FED_GLM_FISHER_GRID caps the row-chunk blocks per panel pair (tests
    // reach several tiles per block at small N with it); read per call
    if (const char* ge = getenv("FED_GLM_FISHER_GRID")) {
        const int v = atoi(ge);
        if (v >= 1 && v < chunks) chunks = v;
    }
    const long long chunk_bytes = (long long)NPP * wrs * PW * PW * sizeof(float);
    if (chunks * chunk_bytes > slab_bytes) chunks = slab_bytes / chunk_bytes;
    if (chunks < 1) return -3;
    const int grid = (int)(chunks * NPP);
    long long wgrid = (n_rows + 7) / 8;
    if (wgrid > 2048) wgrid = 2048;
    if (wgrid < 1) wgrid = 1;

    const LinkParams lp = make_link_params(sigma);
    bool ok;
    if (link == FED_LINK_POISSON)
        ok = dispatch_fs<PoissonLink>(K, grid, (int)wgrid, stream, X, offset_f32, n_rows, beta_f32,
                                      lp, workspace, slab);
    else
        ok = dispatch_fs<GaussianLink>(K, grid, (int)wgrid, stream, X, offset_f32, n_rows,
                                       beta_f32, lp, workspace, slab);
    if (!ok) return -4;
    hipError_t kerr = hipGetLastError();
    if (kerr != hipSuccess) return (int)kerr;

    // few entries (narrow K): more slices of the slab rows per entry
    const int SL = PW >= 64 ? 4 : (PW == 32 ? 16 : 64);
    const long long entries = (long long)NPP * PW * PW;
    const int E = 256 / SL;
    hipLaunchKernelGGL(k_fisher_reduce, dim3((unsigned)((entries + E - 1) / E)), dim3(256), 0,
                       stream, slab, (int)(chunks * wrs), wrs, NP, PW, K, SL, out);
    return (int)hipGetLastError();
}

}  // extern "C"
