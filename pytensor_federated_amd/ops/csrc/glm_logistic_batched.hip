// Batched (16-chain) logistic GLM on CDNA4 (gfx950) matrix cores: the MFMA
// fragment-map probe, the kernels that ship (v3 at K=1024, v2 at K=512, v3s
// as an opt-in) and their dispatcher.
// Every kernel here is covered by the exact-probe tests.  Shared pieces and
// the overview of the GLM units are in fed_common.hpp.
//
// History (ms at 2e6 x 1024 x 16 bf16, profiles/PROFILES.md): v1, a
// double-buffered chunk pipeline that re-reads X for phase B, 1.568; v2,
// v1 plus an XOR bank swizzle and a reverse phase-B chunk walk, 1.035 (the
// 2x-traffic floor; 0.567 at K=512, where it is the default); v3, a
// tile-resident LDS-DMA pipeline that reads X once, 0.878 (~0.95 same-box
// against its successor); v3 on the transpose-read image, 0.89, the K=1024
// default.  The scalar-gather image of v3, its instrumented build and the
// two environment flags that selected them last exist at commit 5e9376b.
// v1 and the flag that selected it (FED_BATCHED_V1) last exist at commit
// ebb4f6a.  The LDS-resident whole-tile variant, which lost its round-1 A/B
// to v1 (no figure recorded), and its flag (FED_BATCHED_LDS) last exist at
// commit 84bf623.

#include "fed_common.hpp"

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_t;
typedef __attribute__((ext_vector_type(4))) float f32x4_t;

// ---------------------------------------------------------------------------
// MFMA fragment-map probe (test-only): D = A[16x32] . B[32x16], bf16->f32.
// Assumed lane mapping (verified on hardware by tests/test_gpu.py):
//   A: row i = lane&15, k = (lane>>4)*8 + j   (8 bf16 per lane)
//   B: col j = lane&15, k = (lane>>4)*8 + jj  (8 bf16 per lane)
//   D: col   = lane&15, row = (lane>>4)*4 + reg
// ---------------------------------------------------------------------------

__global__ __launch_bounds__(64) void k_mfma_probe(
    const unsigned short* __restrict__ A,  // [16][32] bf16 row-major
    const unsigned short* __restrict__ B,  // [32][16] bf16 row-major
    float* __restrict__ D                  // [16][16] f32 row-major
) {
    const int lane = threadIdx.x & 63;
    union { bf16x8_t v; unsigned short u[8]; } a_frag, b_frag;
    const int arow = lane & 15;
    const int k0 = (lane >> 4) * 8;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        a_frag.u[j] = A[arow * 32 + k0 + j];
        b_frag.u[j] = B[(k0 + j) * 16 + (lane & 15)];
    }
    f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a_frag.v, b_frag.v, acc, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = (lane >> 4) * 4 + r;
        const int col = lane & 15;
        D[row * 16 + col] = acc[r];
    }
}

extern "C" int fed_mfma_probe(const void* A, const void* B, void* D, void* stream_v) {
    hipLaunchKernelGGL(k_mfma_probe, dim3(1), dim3(64), 0, (hipStream_t)stream_v,
                       (const unsigned short*)A, (const unsigned short*)B, (float*)D);
    return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------
// Batched logistic GLM: B=16 chains per call on MFMA matrix cores
// ---------------------------------------------------------------------------
//
// Multi-chain MCMC (the reference's pm.sample(cores=N) axis) evaluates 16
// proposal vectors in ONE pass over X:
//
//     Z[rows,16]  = X[rows,K] . Theta[K,16]        (phase A, MFMA)
//     logp[b]    += sum_r  y z - softplus(z)
//     R[rows,16]  = y - sigmoid(Z)
//     G[K,16]    += X^T[K,rows] . R[rows,16]       (phase B, MFMA)
//
// X is HBM-read once per call (v2: k-chunks staged to LDS, phase B
// re-reads the L2-hot chunk; v3/v3s: the tile stays in LDS throughout); at
// B=16 the arithmetic is 4*N*K*B flops -- VALU could not keep up with the
// HBM stream (0.8 TFLOP/call vs ~4 ms of traffic), MFMA makes compute a
// ~10% bystander.  Per-chain cost is ~B x lower than the single-chain
// kernel.
//
// Geometry: block = 256 threads = 4 waves.  v2: row tile 64 (16 rows/wave
// in phase A); K chunked by 128 (each wave owns a 32-col slice in phase B).
// v3/v3s: row tile 32, every wave owns a K slice in both phases.  G
// accumulates in AGPRs (16 tiles x 4 f32/lane/wave at K=1024); per-block
// partials go to an fp32 slab [16 logp | K*16 G], reduced by
// k_colsum_reduce.
//
// Verified fragment maps (fed_mfma_probe): A[i=l&15][k=(l>>4)*8+j],
// B[k=(l>>4)*8+j][j=l&15], D[col=l&15][row=(l>>4)*4+r].

#define BCH 16           // chains per call
#define BL_ROWS 64       // rows per block tile (v2)
#define BL_CHUNK 128     // K columns per chunk (v2)
#define XPAD 8           // X_lds row pad (elems): stride 272 B, b128-clean
#define TPAD 8           // Theta row pad: stride 2064+16 B
#define RPAD 8           // R_T row pad: stride 144 B

union frag_u { bf16x8_t v; unsigned short u[8]; U4 q; };

// ---- pieces every batched kernel shares (all inlined; the kernels differ
// ---- in how X is staged and walked, not in these) ----
// Only what compiles to the same instruction mix as the in-place code is
// shared.  The Theta^T preload loop is not: as a helper it is laid out
// differently (exec-mask handling of the loop exit changes in every kernel),
// so each kernel keeps its own five lines.

// fp32 -> bf16 bits, round to nearest even (R feeds the phase-B MFMA)
__device__ __forceinline__ unsigned short f32_to_bf16_rne_bits(float f) {
    union { float f; unsigned int u; } cv;
    cv.f = f;
    const unsigned int rnd = 0x7fff + ((cv.u >> 16) & 1);
    return (unsigned short)((cv.u + rnd) >> 16);
}

// One valid (row, chain) slot: logp += y z - softplus(z) (stable form),
// returns the residual y - sigmoid(z).  Order: sp, term, residual.
__device__ __forceinline__ float logistic_term_resid(float z, float yv, float& logp) {
    const float sp = fmaxf(z, 0.f) + log1pf(__expf(-fabsf(z)));
    logp += yv * z - sp;
    return yv - 1.f / (1.f + __expf(-z));
}

// Epilogue: per-thread logp partials (chain = thread & 15) -> the block's
// 16 per-chain sums at the head of its slab row.  Returns the G part of
// the row, which each kernel fills from its g_acc tiles by its own column
// map (a shared scatter helper changed the address arithmetic the compiler
// emits for the stores, so those loops stay in the kernels).
template <int K>
__device__ __forceinline__ float* epilogue_logp(float* slab, float* red_lds, float logp) {
    red_lds[threadIdx.x] = logp;
    __syncthreads();
    float* slab_blk = slab + (long long)blockIdx.x * (BCH + (long long)K * BCH);
    if (threadIdx.x < BCH) {
        float s = 0.f;
        for (int i = threadIdx.x; i < 256; i += BCH) s += red_lds[i];
        slab_blk[threadIdx.x] = s;
    }
    return slab_blk + BCH;
}

// ---------------------------------------------------------------------------
// Batched logistic v2: double-buffered chunk pipeline, swizzled LDS
// ---------------------------------------------------------------------------
// A 64-row tile is walked in 128-column chunks through two LDS buffers,
// over BOTH phases: phase A consumes chunks 0..n-1 (Z), phase B consumes
// them again in reverse (G), re-reading X through L2.  One barrier per
// chunk step.  What the measurements fixed (profiles/PROFILES.md; the
// unswizzled forward-walking predecessor measured 1.57 ms, with 10.8% LDS
// bank-conflict cycles from the phase-B transposed u16 reads: rows r/r+8
// land on one bank at the 16B-aligned row stride):
//
//  * load placement: chunk c+1's global loads are issued BEFORE chunk c's
//    MFMAs and written to LDS after them.  That forces the allocator to keep
//    four load register quads alive across the MFMAs, so four loads are in
//    flight.  A write-after-barrier variant (load c+2 right after the
//    staging write) was tried and REVERTED: hipcc coalesced the 4 staging
//    loads into one register quad with a serial s_waitcnt vmcnt(0) per load
//    -- serial HBM round trips, 2.8 ms vs 1.57.
//  * XOR swizzle of the 16-byte group index, key = ((row>>3)&1)<<1 --
//    rows r and r+8 (the colliding pair within a 32-lane half) get their
//    group-bit-1 flipped against each other, separating their banks for
//    the phase-B scalar reads while leaving the b128 write/read patterns
//    near-conflict-free.
//  * edge rows zero-fill by the CONDITIONAL form (zero, then load if the
//    row is in range): an address-clamp variant (branch-free) made hipcc
//    spill the staged loads to scratch with a vmcnt(0) after EACH -- serial
//    HBM round trips (2.8 ms).  With the conditional form the 4 loads stay
//    in 4 register quads, in flight together (verified in the ISA).
//
// Chunk staging: a thread owns rows {st_r0 + 16 rr}, one 16-B group each,
// loaded as one group of four and zero-filled conditionally (both: above).
// Macros, not functions: a function form (U4 (&ld)[4] by reference)
// compiled to a different instruction mix in both instantiations, and this
// code is compiler-sensitive.  They use the kernel's X, n_rows, row0, st_r0,
// ld, x_lds, x_buf and x_stride; `k0` is the thread's column within chunk
// `c`, `lds_col` its swizzled column in the LDS row of buffer `buf`.
#define BL_LOAD_CHUNK(c, k0)                                                    \
    _Pragma("unroll") for (int rr = 0; rr < 4; ++rr) {                          \
        const long long row = row0 + st_r0 + rr * 16;                           \
        ld[rr] = (U4){0, 0, 0, 0};                                              \
        if (row < n_rows)                                                       \
            ld[rr] = *(const U4*)&X[row * (long long)K + (c) * BL_CHUNK + k0];  \
    }
#define BL_WRITE_CHUNK(buf, lds_col)                                            \
    _Pragma("unroll") for (int rr = 0; rr < 4; ++rr)                            \
        *(U4*)&x_lds[(buf) * x_buf + (st_r0 + rr * 16) * x_stride + lds_col] = ld[rr];

template <int K>  // compile-time K: keeps g_acc statically indexed (no
                  // scratch spill -- cdna_hip_programming.md rule 20)
__global__ __launch_bounds__(256) void k_logistic_glm_batched_v2(
    const unsigned short* __restrict__ X,   // [N][K] bf16
    const unsigned short* __restrict__ y,   // [N] bf16
    long long n_rows,
    const unsigned short* __restrict__ theta_t,  // [BCH][K] bf16 (transposed)
    float* __restrict__ slab                     // [grid][BCH + K*BCH]
) {
    const int lane = threadIdx.x & 63;
    const int wid = threadIdx.x >> 6;
    constexpr int n_chunks = K / BL_CHUNK;

    extern __shared__ __attribute__((aligned(16))) char smem[];
    unsigned short* th_lds = (unsigned short*)smem;             // [BCH][K+TPAD]
    const int th_stride = K + TPAD;
    unsigned short* x_lds = th_lds + BCH * th_stride;           // [2][BL_ROWS][BL_CHUNK+XPAD]
    const int x_stride = BL_CHUNK + XPAD;
    const int x_buf = BL_ROWS * x_stride;
    unsigned short* rt_lds = x_lds + 2 * x_buf;                 // [BCH][BL_ROWS+RPAD]
    const int rt_stride = BL_ROWS + RPAD;
    float* y_lds = (float*)(rt_lds + BCH * rt_stride + 8);      // [BL_ROWS]
    float* red_lds = y_lds + BL_ROWS;                           // [256]

    // Theta^T staged once per block (a theta read from global inside the
    // MFMA loop poisons the vmcnt pipeline: its wait is FIFO-ordered after
    // the chunk-prefetch loads, so every chunk step drained its prefetch --
    // measured 2.97 ms vs 1.56 ms with Theta in LDS, and reverted)
    for (int idx = threadIdx.x * 8; idx < BCH * K; idx += 256 * 8) {
        const int b = idx / K;
        const int k = idx % K;
        *(U4*)&th_lds[b * th_stride + k] = *(const U4*)&theta_t[b * K + k];
    }

    f32x4_t g_acc[n_chunks * 2];
#pragma unroll
    for (int t = 0; t < n_chunks * 2; ++t) g_acc[t] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    float logp_acc = 0.f;  // this lane's chain partial (chain = lane&15)

    // staging: thread owns rows {r0, r0+16, r0+32, r0+48}, one 16B group each
    const int st_r0 = threadIdx.x / 16;               // 0..15
    const int st_g = threadIdx.x % 16;                // 16B group within chunk
    const int st_key = ((st_r0 >> 3) & 1) << 1;       // swizzle key (rows +16 share it)
    const long long row_max = n_rows - 1;

    const long long n_tiles = (n_rows + BL_ROWS - 1) / BL_ROWS;
    for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const long long row0 = tile * BL_ROWS;
        if (threadIdx.x < BL_ROWS) {
            const long long r = row0 + threadIdx.x;
            y_lds[threadIdx.x] = r < n_rows ? bf16_bits_to_f32(y[r]) : 0.f;
        }

        U4 ld[4];
        // global loads are linear (coalesced); the XOR swizzle is applied at
        // the LDS WRITE, and compensated at both read sites.

        BL_LOAD_CHUNK(0, st_g * 8)
        BL_WRITE_CHUNK(0, (st_g ^ st_key) * 8)
        int cur = 0;

        // ---- phase A: Z = X . Theta ----
        // The load placement is deliberate (see the notes above the
        // kernel): chunk c+1's loads go out BEFORE chunk c's MFMAs, the
        // LDS write follows them, and that keeps 4 loads in flight.
        f32x4_t z_acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < n_chunks; ++c) {
            __syncthreads();  // buf[cur] visible (and y_lds on c==0)
            if (c + 1 < n_chunks) BL_LOAD_CHUNK(c + 1, st_g * 8)
            const int arow = wid * 16 + (lane & 15);
            const int akey = (((arow >> 3) & 1) << 1);
#pragma unroll
            for (int ks = 0; ks < BL_CHUNK / 32; ++ks) {
                frag_u a, b;
                const int ag = (ks * 4 + (lane >> 4)) ^ akey;
                a.q = *(U4*)&x_lds[cur * x_buf + arow * x_stride + ag * 8];
                const int bk = c * BL_CHUNK + ks * 32 + (lane >> 4) * 8;
                b.q = *(U4*)&th_lds[(lane & 15) * th_stride + bk];
                z_acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.v, b.v, z_acc, 0, 0, 0);
            }
            if (c + 1 < n_chunks) BL_WRITE_CHUNK(cur ^ 1, (st_g ^ st_key) * 8)
            cur ^= 1;
        }

        // ---- logp + R from Z (prefetch chunk n-1 for phase B) ----
        BL_LOAD_CHUNK(n_chunks - 1, st_g * 8)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row_in_wave = (lane >> 4) * 4 + r;
            const int row_in_tile = wid * 16 + row_in_wave;
            const long long row = row0 + row_in_tile;
            const int chain = lane & 15;
            float z = z_acc[r];
            float yv = y_lds[row_in_tile];
            float resid = 0.f;
            if (row < n_rows) resid = logistic_term_resid(z, yv, logp_acc);
            rt_lds[chain * rt_stride + row_in_tile] = f32_to_bf16_rne_bits(resid);
        }
        __syncthreads();  // R complete; x_lds free
        // buffer 0 <- the chunk-(n-1) data loaded above
        BL_WRITE_CHUNK(0, (st_g ^ st_key) * 8)
        cur = 0;

        // ---- phase B: G += X_chunk^T . R, chunks walked in REVERSE ----
        // phase A finished on chunk n-1, so that chunk's lines are the
        // L2-hottest; walking n-1..0 maximizes phase B's L2 hit rate on the
        // re-read (forward order re-read chunk 0 first, the line most
        // likely already evicted).
#pragma unroll
        for (int ci = 0; ci < n_chunks; ++ci) {
            const int c = n_chunks - 1 - ci;
            __syncthreads();
            if (c - 1 >= 0) BL_LOAD_CHUNK(c - 1, st_g * 8)
#pragma unroll
            for (int t2 = 0; t2 < 2; ++t2) {
                const int kcol0 = wid * 32 + t2 * 16;
                f32x4_t acc = g_acc[c * 2 + t2];
#pragma unroll
                for (int rs = 0; rs < 2; ++rs) {
                    frag_u a, b;
                    const int kcol = kcol0 + (lane & 15);
                    const int arow0 = rs * 32 + (lane >> 4) * 8;
                    // all 8 rows of this fragment share (row>>3), so the
                    // swizzle key (and the whole LDS column base) hoists
                    const int bkey = (((arow0 >> 3) & 1) << 1);
                    const int bg = (kcol >> 3) ^ bkey;
                    const unsigned short* col =
                        &x_lds[cur * x_buf + arow0 * x_stride + bg * 8 + (kcol & 7)];
#pragma unroll
                    for (int j = 0; j < 8; ++j)
                        a.u[j] = col[j * x_stride];
                    b.q = *(U4*)&rt_lds[(lane & 15) * rt_stride + rs * 32 + (lane >> 4) * 8];
                    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.v, b.v, acc, 0, 0, 0);
                }
                g_acc[c * 2 + t2] = acc;
            }
            if (c - 1 >= 0) BL_WRITE_CHUNK(cur ^ 1, (st_g ^ st_key) * 8)
            cur ^= 1;
        }
        __syncthreads();  // rt_lds reuse next tile
    }

    // ---- epilogue: block partials -> slab ----
    float* g_slab = epilogue_logp<K>(slab, red_lds, logp_acc);
#pragma unroll
    for (int c = 0; c < n_chunks; ++c) {
#pragma unroll
        for (int t2 = 0; t2 < 2; ++t2) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int kcol = c * BL_CHUNK + wid * 32 + t2 * 16 + (lane >> 4) * 4 + r;
                const int chain = lane & 15;
                g_slab[(long long)kcol * BCH + chain] = g_acc[c * 2 + t2][r];
            }
        }
    }
}

// ---------------------------------------------------------------------------
// Batched logistic v3 / v3s: glds-staged, tile-RESIDENT, no phase-B re-read
// ---------------------------------------------------------------------------
// v2 sits at the 2x-traffic floor (~1.03 ms at 2e6x1024: phase B re-reads X
// from HBM).  v3 removes the re-read: a 32-row x K tile stays resident in
// LDS across BOTH phases.  Staging is global_load_lds (1-KB DMAs, no VGPR
// round trip), pipelined one tile ahead through three 32-KB half-buffers
// with COUNTED vmcnt waits and raw s_barriers (a __syncthreads with a glds
// in flight drains the whole queue).  1 block/CU, contiguous tile ranges.
// The counts (8 DMAs per wave per staged half) hold for full tiles only;
// the problem's tail tile is processed outside the counted pipeline.
//
// Two LDS images.  v3 (K=1024) stores [4][16] subtiles for the hardware
// transpose read (tr_img below).  v3s (K=512) stores swizzled rows, one
// 1-KB DMA per row: the pad-free image (row stride 512 u16 == 0 mod 64
// dwords) would put every row on the same banks, so the SOURCE column
// group of each lane is XOR-permuted by key(row) = rotl4_by2(row & 15):
// 4-bit-injective (phase-A b128 slots stay distinct) and key(r) ^
// key(r+8) == 2 (the phase-B u16 lane-pairs that share a bank mod 8 get
// split by bit1, while bit0 stays free for the kcol-block bit).
//
// Per-wave column split is interleaved across halves (wave w owns cols
// [w*128, w*128+128) of EACH half) so both phases keep all 4 waves busy
// on whichever half is resident, and the h1 buffer can be refilled for
// tile t+1 while phase B finishes tile t's h0 columns.

#define V3_ROWS 32        // rows per tile
#define V3_HALF 512       // columns per half (K = 1024 only)

__device__ __forceinline__ int v3_key(int row) {
    const int x = row & 15;
    return ((x << 2) | (x >> 2)) & 15;  // rotl4 by 2
}

#define V3_ASM_VMCNT(n) asm volatile("s_waitcnt vmcnt(" #n ")" ::: "memory")
#define V3_BARRIER()                                                    \
    do {                                                                \
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");              \
        __builtin_amdgcn_s_barrier();                                   \
    } while (0)

// One 1-KB LDS-DMA; the LDS destination is wave-uniform (m0).
// The DMA is issued by INLINE ASM, not the builtin: hipcc tracks builtin
// glds in its memory model and bundles `s_waitcnt vmcnt(0)` into the
// lgkm wait of EVERY later ds_read that might alias -- which drains the
// cross-tile prefetch at each MFMA (observed in the .s).  The asm form
// leaves its completion entirely to this kernel's hand-counted
// V3_ASM_VMCNT waits (the glds queue shares vmcnt, FIFO).
__device__ __forceinline__ void v3_glds_row(const void* src, unsigned lds_byte_off) {
    // nt: each X line is streamed by exactly one CU exactly once (the
    // tile-resident design's whole point), the guide's nt-weights case
    // (issued->landed -18%).  No "memory" clobber: it would make hipcc
    // bundle a conservative vmcnt(0) into every later ds_read's wait (the
    // exact drain this asm form exists to avoid) -- ordering is carried
    // by the volatile asm barriers (which DO clobber memory).
    asm volatile(
        "s_mov_b32 m0, %0\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %1, off nt"
        :: "s"(lds_byte_off), "v"(src));
}

__device__ __forceinline__ void v3_glds_row_cached(const void* src, unsigned lds_byte_off) {
    asm volatile(
        "s_mov_b32 m0, %0\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %1, off"
        :: "s"(lds_byte_off), "v"(src));
}

// load one y value through a HIDDEN asm global load: it rides the same
// vmcnt queue as the tile DMAs (so the [4] counted wait covers it) and,
// unlike an ordinary tracked load, does not make hipcc insert a
// conservative vmcnt(0) drain at the use.  OOB rows clamp the address
// (uniform issue keeps the per-wave ledger exact); the caller masks the
// value.  (A 1-byte-per-lane LDS-DMA variant of this was tried first and
// produced wrong y values -- ubyte DMA lane addressing did not match the
// lane*size model; reverted to register loads.)
__device__ __forceinline__ unsigned v3_load_y_asm(const unsigned short* addr) {
    unsigned v;
    asm volatile("global_load_ushort %0, %1, off"
                 : "=v"(v) : "v"(addr));
    return v;
}

// Swizzled-row image (v3s): stage rows [8w, 8w+8) of one 512-col half, one
// 1-KB LDS-DMA per row, source columns pre-swizzled per lane.
__device__ __forceinline__ void v3_stage_half(
    const unsigned short* __restrict__ X, long long n_rows, int K,
    long long row0, int colbase, unsigned short* half_buf,
    const char* smem_base, int wid, int lane, int nt_on
) {
#pragma unroll
    for (int rr = 0; rr < 8; ++rr) {
        const int r = wid * 8 + rr;
        const long long grow = row0 + r;
        unsigned short* dst = half_buf + r * V3_HALF;
        if (grow < n_rows) {
            const unsigned short* src =
                &X[grow * (long long)K + colbase + ((lane ^ v3_key(r)) * 8)];
            // the row base is wave-uniform by construction; readfirstlane
            // makes that provable so the asm "s" constraint gets an SGPR
            const unsigned off = __builtin_amdgcn_readfirstlane(
                (unsigned)((const char*)dst - smem_base));
            if (nt_on & 1) v3_glds_row(src, off);
            else v3_glds_row_cached(src, off);
        } else {
            *(U4*)&dst[lane * 8] = (U4){0, 0, 0, 0};
        }
    }
}

// Transpose-read image (v3): one 1-KB DMA = 4 rows x 128 cols landing as 8
// contiguous [4][16] subtiles; per wave 8 DMAs (row-groups 2w..2w+1 x 4
// col-octets), the same count as v3_stage_half, so one set of vmcnt
// ledgers serves both images on full tiles.  On the tail tile
// a wave issues 4 DMAs per fully valid row-group and none for an edge one
// (v3_stage_half: one per valid row), so the kernel keeps the tail tile
// out of the counted pipeline.  Lane n supplies the source of
// image element n*8: subtile s = n>>3, row j = (n&7)>>1, col-half h = n&1.
__device__ __forceinline__ void tr_stage_half(
    const unsigned short* __restrict__ X, long long n_rows, int K,
    long long row0, int colbase, unsigned short* half_buf,
    const char* smem_base, int wid, int lane, int nt_on
) {
#pragma unroll
    for (int rr = 0; rr < 8; ++rr) {
        const int rg = wid * 2 + (rr >> 2);   // row-group (4 rows) 0..7
        const int oct = rr & 3;               // col-octet (128 cols) 0..3
        const long long grow0 = row0 + rg * 4;
        unsigned short* dst = half_buf + (rg * 32 + oct * 8) * 64;
        const int s = lane >> 3;
        const int j = (lane & 7) >> 1;
        const int h = lane & 1;
        if (grow0 + 4 <= n_rows) {
            const unsigned short* srcp =
                &X[(grow0 + j) * (long long)K + colbase + oct * 128 + s * 16 + h * 8];
            const unsigned off = __builtin_amdgcn_readfirstlane(
                (unsigned)((const char*)dst - smem_base));
            if (nt_on & 1) v3_glds_row(srcp, off);
            else v3_glds_row_cached(srcp, off);
        } else {
            // edge row-group: zero-fill, then guarded plain writes of the
            // in-range rows through the subtiled mapping
            *(U4*)&dst[lane * 8] = (U4){0, 0, 0, 0};
            const long long grow = grow0 + j;
            if (grow < n_rows) {
                *(U4*)&dst[(s * 64) + (j * 16) + h * 8] =
                    *(const U4*)&X[grow * (long long)K + colbase + oct * 128 +
                                   s * 16 + h * 8];
            }
        }
    }
}

// Small-K sibling of v3 (K <= 512, multiple of 128): a whole 32-row x K
// tile is ONE <=32-KB buffer, so the pipeline is a plain 3-buffer rotation
// with prefetch depth TWO tiles (the K=1024 kernel must split tiles into
// column halves to fit; here each buffer is self-sufficient, which also
// lets phase A finish Z in one sweep).  Staging, swizzle, hidden y loads
// and the counted-vmcnt discipline are identical to v3.
template <int K>
__global__ __launch_bounds__(256) void k_logistic_glm_batched_v3s(
    const unsigned short* __restrict__ X,   // [N][K] bf16
    const unsigned short* __restrict__ y,   // [N] bf16
    long long n_rows,
    const unsigned short* __restrict__ theta_t,  // [16][K] bf16
    float* __restrict__ slab,                    // [grid][16 + K*16]
    int nt_on                                    // nt on the tile DMAs (A/B)
) {
    const int lane = threadIdx.x & 63;
    const int wid = threadIdx.x >> 6;
    constexpr int QC = K / 4;        // columns per wave quarter
    constexpr int NKS = QC / 32;     // phase-A MFMA steps per quarter
    constexpr int NT2 = QC / 16;     // phase-B column tiles per quarter
    constexpr int TBUF = V3_ROWS * K;  // u16 per tile buffer

    extern __shared__ __attribute__((aligned(16))) char smem[];
    unsigned short* th_lds = (unsigned short*)smem;        // [16][K+TPAD]
    const int th_stride = K + TPAD;
    unsigned short* x_base = th_lds + BCH * th_stride;     // 3 x [32][K]
    unsigned short* rt_lds = x_base + 3 * TBUF;            // [16][32+RPAD]
    const int rt_stride = V3_ROWS + RPAD;
    float* zc_lds = (float*)(rt_lds + BCH * rt_stride);    // [4][32][16]
    float* red_lds = zc_lds + 4 * V3_ROWS * BCH;           // [256]

    for (int idx = threadIdx.x * 8; idx < BCH * K; idx += 256 * 8) {
        const int b = idx / K;
        const int k = idx % K;
        *(U4*)&th_lds[b * th_stride + k] = *(const U4*)&theta_t[b * K + k];
    }
    __syncthreads();

    f32x4_t g_acc[NT2];
#pragma unroll
    for (int t = 0; t < NT2; ++t) g_acc[t] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    float logp0 = 0.f, logp1 = 0.f;

    const long long n_tiles = (n_rows + V3_ROWS - 1) / V3_ROWS;
    const long long tpb = (n_tiles + gridDim.x - 1) / gridDim.x;
    const long long t_begin = blockIdx.x * tpb;
    const long long t_end = t_begin + tpb < n_tiles ? t_begin + tpb : n_tiles;

    // stage one whole tile into buffer `buf`: at K=512 one row is exactly
    // the 1-KB glds span (row stride = K*2 = 1024 B), so a tile is staged
    // as one v3 half at column 0; fully out-of-range rows zero-fill.
    static_assert(K == V3_HALF, "v3s is instantiated for the padded K=512 granule");
    auto stage_tile = [&](long long row0, int buf) {
        v3_stage_half(X, n_rows, K, row0, 0, x_base + buf * TBUF, smem, wid, lane, nt_on);
    };

    // The counted waits below assume 8 DMAs per wave per staged tile; the
    // problem's TAIL tile stages one DMA per VALID row (0..8 per wave), so
    // a vmcnt(8) counted against it waits for too little.  As in v3 it is
    // kept out of the counted pipeline: pass 0 runs this block's FULL tiles,
    // pass 1 the tail tile alone (a one-tile range only ever waits with
    // vmcnt(0)).  Both ranges are block-uniform.
    const long long n_full = n_rows / V3_ROWS;  // tiles with every row valid
#pragma unroll 1
    for (int pass = 0; pass < 2; ++pass) {
        const long long p_begin = pass == 0 ? t_begin : (t_begin > n_full ? t_begin : n_full);
        const long long p_end = pass == 0 ? (t_end < n_full ? t_end : n_full) : t_end;
        if (p_begin >= p_end) continue;
        // pass 1 restages buffer 0: pass 0 ended drained and behind its
        // closing barrier, so the buffer is free
        stage_tile(p_begin * V3_ROWS, 0);
        if (p_begin + 1 < p_end) stage_tile((p_begin + 1) * V3_ROWS, 1);

#pragma unroll 1
        for (long long tile = p_begin; tile < p_end; ++tile) {
            const long long row0 = tile * V3_ROWS;
            unsigned short* xb = x_base + (int)((tile - p_begin) % 3) * TBUF;
            const bool more1 = tile + 1 < p_end;
            const bool more2 = tile + 2 < p_end;

            // [a] own tile's DMAs complete; newer: t+1's (8/RPD) if issued
            if (more1) V3_ASM_VMCNT(8); else V3_ASM_VMCNT(0);
            V3_BARRIER();
            // y loads (hidden) BEFORE the prefetch, as in v3
            const long long ymax = n_rows - 1;
            long long yr0 = row0 + (threadIdx.x >> 4);
            long long yr1 = row0 + 16 + (threadIdx.x >> 4);
            const unsigned yb0 = v3_load_y_asm(y + (yr0 > ymax ? ymax : yr0));
            const unsigned yb1 = v3_load_y_asm(y + (yr1 > ymax ? ymax : yr1));
            if (more2) stage_tile((tile + 2) * V3_ROWS, (int)((tile + 2 - p_begin) % 3));

            // ---- phase A: complete Z over this wave's K-quarter ----
            f32x4_t z0 = {0.f, 0.f, 0.f, 0.f}, z1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < NKS; ++ks) {
                const int kc = wid * QC + ks * 32;
                frag_u bf, a0, a1;
                const int g = (kc >> 3) + (lane >> 4);
                const int arow0 = lane & 15;
                const int arow1 = 16 + (lane & 15);
                a0.q = *(U4*)&xb[arow0 * K + ((g ^ v3_key(arow0)) * 8)];
                a1.q = *(U4*)&xb[arow1 * K + ((g ^ v3_key(arow1)) * 8)];
                const int bk = kc + (lane >> 4) * 8;
                bf.q = *(U4*)&th_lds[(lane & 15) * th_stride + bk];
                z0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0.v, bf.v, z0, 0, 0, 0);
                z1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1.v, bf.v, z1, 0, 0, 0);
            }
            {
                float* zc = zc_lds + wid * V3_ROWS * BCH;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    zc[((lane >> 4) * 4 + r) * BCH + (lane & 15)] = z0[r];
                    zc[(16 + (lane >> 4) * 4 + r) * BCH + (lane & 15)] = z1[r];
                }
            }
            // y complete: newer ops are the prefetch's DMAs only
            if (more2) V3_ASM_VMCNT(8); else V3_ASM_VMCNT(0);
            V3_BARRIER();
            {
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    const int slot = threadIdx.x + s * 256;
                    const int row = slot >> 4;
                    const int chain = slot & 15;
                    float z = 0.f;
#pragma unroll
                    for (int w = 0; w < 4; ++w)
                        z += zc_lds[(w * V3_ROWS + row) * BCH + chain];
                    const long long grow = row0 + row;
                    float resid = 0.f;
                    if (grow < n_rows) {
                        const float yv = bf16_bits_to_f32(
                            (unsigned short)(s == 0 ? yb0 : yb1));
                        resid = logistic_term_resid(z, yv, s == 0 ? logp0 : logp1);
                    }
                    rt_lds[chain * rt_stride + row] = f32_to_bf16_rne_bits(resid);
                }
            }
            V3_BARRIER();  // R visible

            // ---- phase B over this wave's quarter ----
#pragma unroll
            for (int t2 = 0; t2 < NT2; ++t2) {
                const int kc = wid * QC + t2 * 16;
                const int kcol = kc + (lane & 15);
                f32x4_t acc = g_acc[t2];
                frag_u a, b;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int row = (lane >> 4) * 8 + j;
                    a.u[j] = xb[row * K +
                                (((kcol >> 3) ^ v3_key(row)) * 8) + (kcol & 7)];
                }
                b.q = *(U4*)&rt_lds[(lane & 15) * rt_stride + (lane >> 4) * 8];
                g_acc[t2] =
                    __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.v, b.v, acc, 0, 0, 0);
            }
            V3_BARRIER();  // xb free for the t+3 prefetch next iteration
        }
    }

    // ---- epilogue ----
    __syncthreads();
    float* g_slab = epilogue_logp<K>(slab, red_lds, logp0 + logp1);
#pragma unroll
    for (int t2 = 0; t2 < NT2; ++t2) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int kcol = wid * QC + t2 * 16 + (lane >> 4) * 4 + r;
            const int chain = lane & 15;
            g_slab[(long long)kcol * BCH + chain] = g_acc[t2][r];
        }
    }
}

// v3's LDS image: X stored as row-major [4][16] subtiles so phase-B
// fragments come from gfx950's hardware transpose-read (probe-verified
// semantics, scripts/tr_probe.hip: each 16-lane
// group hands lane (l&15) COLUMN l&15 of the 64-elem tile its addresses
// cover, elems {base + (l&15) + 16j}).  Element offset of (row, col)
// within a 32-row x 512-col half:
__device__ __forceinline__ int tr_img(int row, int col) {
    return (((row >> 2) * 32 + (col >> 4)) << 6) + ((row & 3) << 4) + (col & 15);
}

// The kernel below has two phase-A bodies (h0, h1) and two phase-B bodies
// (h1, h0), all on the one [4][16]-subtile image.  They are NOT factored:
// as helpers taking the half buffer and the g_acc offset (or as one body
// in an unrolled two-step loop) they compile to different address
// arithmetic, wait counts and register counts, and this kernel is only
// changed when the result can be shown unchanged.  A fix to the body for
// one half goes into the body for the other half as well.
__global__ __launch_bounds__(256) void k_logistic_glm_batched_v3(
    const unsigned short* __restrict__ X,   // [N][1024] bf16
    const unsigned short* __restrict__ y,   // [N] bf16
    long long n_rows,
    const unsigned short* __restrict__ theta_t,  // [16][1024] bf16
    float* __restrict__ slab,                    // [grid][16 + 1024*16]
    int nt_on                                    // bit0: nt on the tile DMAs (A/B)
) {
    constexpr int K = 2 * V3_HALF;
    const int lane = threadIdx.x & 63;
    const int wid = threadIdx.x >> 6;

    extern __shared__ __attribute__((aligned(16))) char smem[];
    unsigned short* th_lds = (unsigned short*)smem;        // [16][K+TPAD]
    const int th_stride = K + TPAD;
    // three half buffers live at x_base + {0,1,2}*HBUF; they are addressed
    // by OFFSET so every access provably derives from the __shared__ base
    // (a pointer array indexed at runtime loses the address-space
    // inference and hipcc emits flat_load for what should be ds_read)
    constexpr int HBUF = V3_ROWS * V3_HALF;
    unsigned short* x_base = th_lds + BCH * th_stride;     // 3 x [32][512]
    unsigned short* rt_lds = x_base + 3 * HBUF;            // [16][32+RPAD]
    const int rt_stride = V3_ROWS + RPAD;
    float* zc_lds = (float*)(rt_lds + BCH * rt_stride);    // [4][32][16]
    float* red_lds = zc_lds + 4 * V3_ROWS * BCH;           // [256]

    // ---- stage Theta^T once (ordinary loads; BEFORE any glds) ----
    for (int idx = threadIdx.x * 8; idx < BCH * K; idx += 256 * 8) {
        const int b = idx / K;
        const int k = idx % K;
        *(U4*)&th_lds[b * th_stride + k] = *(const U4*)&theta_t[b * K + k];
    }
    __syncthreads();

    f32x4_t g_acc[16];
#pragma unroll
    for (int t = 0; t < 16; ++t) g_acc[t] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    float logp0 = 0.f, logp1 = 0.f;  // this thread's two (row, chain) slots

    // contiguous tile range per block (L2 locality + equal glds ledgers)
    const long long n_tiles = (n_rows + V3_ROWS - 1) / V3_ROWS;
    const long long tpb = (n_tiles + gridDim.x - 1) / gridDim.x;
    const long long t_begin = blockIdx.x * tpb;
    const long long t_end = t_begin + tpb < n_tiles ? t_begin + tpb : n_tiles;

    // The counted vmcnt waits of the tile loop assume 8 DMAs per wave per
    // staged half.  The problem's TAIL tile (fewer than V3_ROWS valid rows)
    // breaks that: a wave issues 4 DMAs per fully valid row-group and fills
    // an edge row-group with LDS stores, so it owns 0, 4 or 8 -- a vmcnt(8)
    // counted against such a half waits for too little and phase A may read
    // rows that have not landed.  The tail tile therefore never enters the
    // counted pipeline: pass 0 runs this block's FULL tiles with the exact
    // ledger, pass 1 runs the tail tile (owned by one block) on its own,
    // fully drained before its first gate.  Both ranges are block-uniform.
    const long long n_full = n_rows / V3_ROWS;  // tiles with every row valid
#pragma unroll 1
    for (int pass = 0; pass < 2; ++pass) {
        const long long p_begin = pass == 0 ? t_begin : (t_begin > n_full ? t_begin : n_full);
        const long long p_end = pass == 0 ? (t_end < n_full ? t_end : n_full) : t_end;
        if (p_begin >= p_end) continue;
        // pass 1 restages buffers 0/1: every wave must be done with pass 0's
        // phase-B reads (pass 0 ends fully drained: its last [4] is vmcnt(0))
        if (pass) V3_BARRIER();
        // prologue: stage tile p_begin fully.  h0 buffers alternate 0/2,
        // h1 lives in buffer 1.
        tr_stage_half(X, n_rows, K, p_begin * V3_ROWS, 0, x_base, smem, wid, lane, nt_on);
        tr_stage_half(X, n_rows, K, p_begin * V3_ROWS, V3_HALF, x_base + HBUF, smem, wid, lane,
                      nt_on);
        // the tail tile's short halves cannot be counted: drain them here,
        // which makes its gate [1] trivially true
        if (pass) V3_ASM_VMCNT(0);

        int h0sel = 0;  // buffer index (0 or 2) holding the CURRENT tile's h0
#pragma unroll 1
        for (long long tile = p_begin; tile < p_end; ++tile) {
            const long long row0 = tile * V3_ROWS;
            unsigned short* h0 = x_base + h0sel * HBUF;
            unsigned short* h1 = x_base + HBUF;
            unsigned short* h0n = x_base + (h0sel ^ 2) * HBUF;  // next tile's h0
            const bool more = tile + 1 < p_end;

            // [1] own h0 DMAs done (h1's 8 may stay in flight), all waves
            V3_ASM_VMCNT(8);
            V3_BARRIER();
            // this thread's two y values (R-step slots), hidden loads on
            // the same queue, issued BEFORE the h0 prefetch so the [4]
            // counted wait (which leaves only the prefetch outstanding)
            // provably covers them
            const long long ymax = n_rows - 1;
            long long yr0 = row0 + (threadIdx.x >> 4);
            long long yr1 = row0 + 16 + (threadIdx.x >> 4);
            const unsigned yb0 = v3_load_y_asm(y + (yr0 > ymax ? ymax : yr0));
            const unsigned yb1 = v3_load_y_asm(y + (yr1 > ymax ? ymax : yr1));
            // [2] prefetch next tile's h0 as deep as possible
            if (more)
                tr_stage_half(X, n_rows, K, row0 + V3_ROWS, 0, h0n, smem, wid, lane, nt_on);

            // ---- phase A on h0: z += X[:, w*128 .. +128) . theta ----
            f32x4_t z0 = {0.f, 0.f, 0.f, 0.f}, z1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                const int kc = wid * 128 + ks * 32;  // column in half
                frag_u b0f, b1f, a0, a1;
                const int g = (kc >> 3) + (lane >> 4);  // 16B group in half
                const int arow0 = lane & 15;            // rows 0..15
                const int arow1 = 16 + (lane & 15);     // rows 16..31
                a0.q = *(U4*)&h0[tr_img(arow0, g * 8)];
                a1.q = *(U4*)&h0[tr_img(arow1, g * 8)];
                const int bk = kc + (lane >> 4) * 8;    // theta col (h0)
                b0f.q = *(U4*)&th_lds[(lane & 15) * th_stride + bk];
                z0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0.v, b0f.v, z0, 0, 0, 0);
                b1f.q = b0f.q;
                z1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1.v, b1f.v, z1, 0, 0, 0);
            }
            // [4] own h1 DMAs + y loads done.  The count must match what
            // was actually issued after them: 8 prefetch DMAs on interior
            // tiles (the prefetched tile is always a full one -- the tail
            // tile is kept out of this pass), NOTHING on the last tile (an
            // unconditional vmcnt(8) there would leave h1/y unwaited -- a
            // timing-dependent race).
            if (more) V3_ASM_VMCNT(8); else V3_ASM_VMCNT(0);
            V3_BARRIER();
            // ---- phase A on h1 ----
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                const int kc = wid * 128 + ks * 32;
                frag_u bf, a0, a1;
                const int g = (kc >> 3) + (lane >> 4);
                const int arow0 = lane & 15;
                const int arow1 = 16 + (lane & 15);
                a0.q = *(U4*)&h1[tr_img(arow0, g * 8)];
                a1.q = *(U4*)&h1[tr_img(arow1, g * 8)];
                const int bk = V3_HALF + kc + (lane >> 4) * 8;  // theta col (h1)
                bf.q = *(U4*)&th_lds[(lane & 15) * th_stride + bk];
                z0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0.v, bf.v, z0, 0, 0, 0);
                z1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1.v, bf.v, z1, 0, 0, 0);
            }
            // ---- combine the 4 waves' z quarters; logp + R ----
            {
                float* zc = zc_lds + wid * V3_ROWS * BCH;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    zc[((lane >> 4) * 4 + r) * BCH + (lane & 15)] = z0[r];
                    zc[(16 + (lane >> 4) * 4 + r) * BCH + (lane & 15)] = z1[r];
                }
            }
            V3_BARRIER();
            {
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    const int slot = threadIdx.x + s * 256;
                    const int row = slot >> 4;      // 0..31
                    const int chain = slot & 15;
                    float z = 0.f;
#pragma unroll
                    for (int w = 0; w < 4; ++w)
                        z += zc_lds[(w * V3_ROWS + row) * BCH + chain];
                    const long long grow = row0 + row;
                    float resid = 0.f;
                    if (grow < n_rows) {
                        const float yv = bf16_bits_to_f32(
                            (unsigned short)(s == 0 ? yb0 : yb1));
                        resid = logistic_term_resid(z, yv, s == 0 ? logp0 : logp1);
                    }
                    rt_lds[chain * rt_stride + row] = f32_to_bf16_rne_bits(resid);
                }
            }
            V3_BARRIER();  // R visible

            // ---- phase B, h1 columns first (frees h1 for the refill) ----
#pragma unroll
            for (int t2 = 0; t2 < 8; ++t2) {
                const int kc = wid * 128 + t2 * 16;       // column in half
                f32x4_t acc = g_acc[8 + t2];
                frag_u a, b;
                // two hardware transpose reads: lane (l&15) gets column
                // kc+(l&15) for rows (l>>4)*8..+3 and +4..+7
                const unsigned base0 = (unsigned)((const char*)&h1[
                    tr_img((lane >> 4) * 8, kc)] - smem) + (lane & 15) * 8u;
                const unsigned base1 = (unsigned)((const char*)&h1[
                    tr_img((lane >> 4) * 8 + 4, kc)] - smem) + (lane & 15) * 8u;
                unsigned long long v0, v1;
                asm volatile(
                    "ds_read_b64_tr_b16 %0, %2\n\t"
                    "ds_read_b64_tr_b16 %1, %3\n\t"
                    "s_waitcnt lgkmcnt(0)"
                    : "=v"(v0), "=v"(v1) : "v"(base0), "v"(base1) : "memory");
                ((unsigned long long*)a.u)[0] = v0;
                ((unsigned long long*)a.u)[1] = v1;
                b.q = *(U4*)&rt_lds[(lane & 15) * rt_stride + (lane >> 4) * 8];
                g_acc[8 + t2] =
                    __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.v, b.v, acc, 0, 0, 0);
            }
            V3_BARRIER();  // everyone done reading h1
            // [6] refill h1 with the NEXT tile's second half
            if (more)
                tr_stage_half(X, n_rows, K, row0 + V3_ROWS, V3_HALF, h1, smem, wid, lane, nt_on);

            // ---- phase B, h0 columns ----
#pragma unroll
            for (int t2 = 0; t2 < 8; ++t2) {
                const int kc = wid * 128 + t2 * 16;
                f32x4_t acc = g_acc[t2];
                frag_u a, b;
                // two hardware transpose reads, as for h1
                const unsigned base0 = (unsigned)((const char*)&h0[
                    tr_img((lane >> 4) * 8, kc)] - smem) + (lane & 15) * 8u;
                const unsigned base1 = (unsigned)((const char*)&h0[
                    tr_img((lane >> 4) * 8 + 4, kc)] - smem) + (lane & 15) * 8u;
                unsigned long long v0, v1;
                asm volatile(
                    "ds_read_b64_tr_b16 %0, %2\n\t"
                    "ds_read_b64_tr_b16 %1, %3\n\t"
                    "s_waitcnt lgkmcnt(0)"
                    : "=v"(v0), "=v"(v1) : "v"(base0), "v"(base1) : "memory");
                ((unsigned long long*)a.u)[0] = v0;
                ((unsigned long long*)a.u)[1] = v1;
                b.q = *(U4*)&rt_lds[(lane & 15) * rt_stride + (lane >> 4) * 8];
                g_acc[t2] =
                    __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.v, b.v, acc, 0, 0, 0);
            }
            h0sel ^= 2;
        }
    }

    // ---- epilogue: block partials -> slab (layout shared with v2) ----
    // the two slots of one thread are chains (t&15) and ((t+256)&15) == same
    // chain, different rows -- so the plain per-chain strided sum works
    __syncthreads();
    float* g_slab = epilogue_logp<K>(slab, red_lds, logp0 + logp1);
#pragma unroll
    for (int half = 0; half < 2; ++half) {
#pragma unroll
        for (int t2 = 0; t2 < 8; ++t2) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int kcol = half * V3_HALF + wid * 128 + t2 * 16 +
                                 (lane >> 4) * 4 + r;
                const int chain = lane & 15;
                g_slab[(long long)kcol * BCH + chain] = g_acc[half * 8 + t2][r];
            }
        }
    }
}

// ---------------------------------------------------------------------------
// Dispatcher
// ---------------------------------------------------------------------------

static bool env_flag(const char* name, bool dflt) {
    const char* e = getenv(name);
    return e ? atoi(e) != 0 : dflt;
}

extern "C" int fed_logistic_glm_batched(
    const void* X, const void* y, long long n_rows, int K,
    const void* theta_t_bf16,  // [16][K] bf16, transposed theta
    double* out,               // fp64[16 + K*16]: [logp[16] | G[K][16]]
    float* workspace, long long ws_bytes,
    void* stream_v
) {
    hipStream_t stream = (hipStream_t)stream_v;
    if (K != 512 && K != 1024) return -4;

    // Variant.  v3 (glds tile-resident, 1x HBM traffic) is the default at
    // K=1024: 0.89 ms vs v2's 1.035 at 2e6x1024x16.  At K=512 the chunked
    // v2 stays default: its 64-KB tiles already re-read through L2
    // (measured 0.567 ms ~= the 1x floor vs v3s 0.645 at 2e6x512 --
    // raw_r2/r2c12); FED_BATCHED_V3=1/0 forces either way.
    const bool v3 = env_flag("FED_BATCHED_V3", K == 1024);

    // Grid.  v2 runs 2 blocks/CU (71 KB LDS); 512 blocks covers every CU
    // twice.  FED_BATCHED_GRID overrides for the L2-residency A/B: at 256
    // (1 block/CU) a block's whole 128 KB tile fits its XCD L2 share, so
    // phase B's re-read can hit L2 instead of HBM -- at the cost of half
    // the waves hiding phase A's stream latency.  v3/v3s hold one block
    // per CU.
    int cap = 512;
    if (const char* ge = getenv("FED_BATCHED_GRID")) {
        int v = atoi(ge);
        if (v >= 16 && v <= 768) cap = v;
    }
    int grid = pick_grid(n_rows / BL_ROWS + 1, 1);
    if (grid > cap) grid = cap;
    const long long slab_cols = BCH + (long long)K * BCH;
    if ((long long)grid * slab_cols * 4 > ws_bytes)
        grid = (int)(ws_bytes / (slab_cols * 4));
    if (grid < 1) return -3;
    if (v3 && grid > 256) grid = 256;

    // Dynamic LDS: u16 elements, then fp32 words, then alignment slack.
    int lds_bytes;
    if (v3)  // Theta, 3 half/tile buffers, R^T | zc, red
        lds_bytes = (BCH * (K + TPAD) + 3 * V3_ROWS * V3_HALF + BCH * (V3_ROWS + RPAD)) * 2 +
                    (4 * V3_ROWS * BCH + 256) * 4 + 64;
    else  // v2: Theta, 2 chunk buffers, R^T | y, red
        lds_bytes = (BCH * (K + TPAD) + 2 * BL_ROWS * (BL_CHUNK + XPAD) +
                     BCH * (BL_ROWS + RPAD) + 8) * 2 +
                    (BL_ROWS + 256) * 4 + 64;

#define LAUNCH_BATCHED(kern, ...)                                                     \
    hipLaunchKernelGGL((kern), dim3(grid), dim3(256), lds_bytes, stream,              \
                       (const unsigned short*)X, (const unsigned short*)y, n_rows,    \
                       (const unsigned short*)theta_t_bf16, workspace, ##__VA_ARGS__)

    if (v3) {
        const int nt_on = env_flag("FED_V3_NT", true);  // stream-once data: nt default
        if (K == 1024) LAUNCH_BATCHED(k_logistic_glm_batched_v3, nt_on);
        else LAUNCH_BATCHED(k_logistic_glm_batched_v3s<512>, nt_on);
    } else {
        if (K == 1024) LAUNCH_BATCHED(k_logistic_glm_batched_v2<1024>);
        else LAUNCH_BATCHED(k_logistic_glm_batched_v2<512>);
    }
#undef LAUNCH_BATCHED
    hipError_t kerr = hipGetLastError();
    if (kerr != hipSuccess) return (int)kerr;

    // slab -> out, zeroed first: the reduce kernel accumulates with atomics
    // when it runs more than one chunk
    hipError_t merr = hipMemsetAsync(out, 0, slab_cols * 8, stream);
    if (merr != hipSuccess) return (int)merr;
    return launch_colsum_reduce(workspace, grid, (int)slab_cols, out, stream);
}
