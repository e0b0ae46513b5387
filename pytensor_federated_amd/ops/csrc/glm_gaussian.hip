// Gaussian linear model on CDNA4 (gfx950): the fused logp+grad kernel and its
// C entry points, result publishing, the multi-shard engine, the device-
// buffer IPC plumbing and the persistent evaluation server.  Shared pieces
// and the overview of the GLM units are in fed_common.hpp.

#include "fed_common.hpp"

// ---------------------------------------------------------------------------
// Gaussian linear regression: fused logp + d/da + d/db
// ---------------------------------------------------------------------------


// Shared element loop for the gaussian reductions.  Mixed precision: the
// residual r is computed in f64 (an f32 pred carries a systematic rounding
// bias that pollutes the cancellation-heavy sum(r) -- measured ~1e-3
// relative at N=1e7), but the r^2 / r*x PRODUCTS accumulate in f32: their
// rounding is uncorrelated (CLT-cancelling), and per-lane spans are short
// before the f64 cross-lane tree.  Saves ~1/3 of the per-element f64 VALU.
//
// One lane's running sums.  The fused kernel and the persistent server both
// feed it the same elements in the same order (vector i of a lane is global
// vector gid + i*gstride, then the scalar tail), so at a given grid they
// return the same bits.
template <typename T>
struct GaussLaneSums {
    using TR = VecTraits<T>;
    using A = typename TR::acc_t;
    static constexpr int VEC = TR::VEC;
    double sr = 0;
    float srx = 0.f, sr2 = 0.f;
    double srx_d = 0, sr2_d = 0;
    long long lane_iters = 0;

    // The multiply-adds are spelled out instead of left to contraction.  The
    // compiler's choice depends on the loop around them: it fused all but
    // one in the streaming loop and a different set in the unrolled
    // resident walk, so the two rounded differently.  What the streaming
    // loop has always computed is now explicit: every multiply-add is an
    // fma, except that the f32 products of the SECOND element of a bf16
    // vector are rounded before they are added (SPLIT).
    template <bool SPLIT = false>
    __device__ __forceinline__ void element(A xj, A yj, double a, double b) {
        const double xd = (double)xj;
        const double r = (double)yj - __builtin_fma(b, xd, a);
        sr += r;
        if constexpr (sizeof(A) == 8) {  // f64 inputs: full f64 products
            srx_d = __builtin_fma(r, xd, srx_d);
            sr2_d = __builtin_fma(r, r, sr2_d);
        } else if constexpr (SPLIT) {
#pragma clang fp contract(off)
            const float r32 = (float)r;
            const float rx = r32 * (float)xd;
            const float rr = r32 * r32;
            srx += rx;
            sr2 += rr;
        } else {
            const float r32 = (float)r;
            srx = __builtin_fmaf(r32, (float)xd, srx);
            sr2 = __builtin_fmaf(r32, r32, sr2);
        }
    }

    // one 16-byte vector of x and of y = one lane iteration
    __device__ __forceinline__ void vector(const A* xv, const A* yv, double a, double b) {
        element(xv[0], yv[0], a, b);
        element<VEC == 8>(xv[1], yv[1], a, b);
#pragma unroll
        for (int j = 2; j < VEC; ++j) element(xv[j], yv[j], a, b);
        // bound the f32 partial span (keeps rounding growth ~sqrt(span))
        if (((++lane_iters) & 255) == 0) {
            srx_d += (double)srx;
            sr2_d += (double)sr2;
            srx = 0.f;
            sr2 = 0.f;
        }
    }

    // grid-stride sweep over vectors first, first+gstride, ... < nvec
    __device__ __forceinline__ void stream(
        const T* __restrict__ x, const T* __restrict__ y, long long nvec,
        long long first, long long gstride, double a, double b
    ) {
        A xv[VEC], yv[VEC];
        for (long long i = first; i < nvec; i += gstride) {
            TR::load(x + i * VEC, xv);
            TR::load(y + i * VEC, yv);
            vector(xv, yv, a, b);
        }
    }

    // the n % VEC rows after the last whole vector
    __device__ __forceinline__ void tail(
        const T* __restrict__ x, const T* __restrict__ y, long long n,
        long long gid, long long gstride, double a, double b
    ) {
        for (long long i = (n / VEC) * VEC + gid; i < n; i += gstride)
            element(TR::get(x, i), TR::get(y, i), a, b);
    }

    __device__ __forceinline__ void finish(double& sr_out, double& srx_out, double& sr2_out) const {
        sr_out = sr;
        srx_out = srx_d + (double)srx;
        sr2_out = sr2_d + (double)sr2;
    }
};

template <typename T>
__device__ __forceinline__ void gauss_accumulate(
    const T* __restrict__ x, const T* __restrict__ y, long long n,
    long long gid, long long gstride, double a, double b,
    double& sr_out, double& srx_out, double& sr2_out
) {
    GaussLaneSums<T> s;
    s.stream(x, y, n / VecTraits<T>::VEC, gid, gstride, a, b);
    s.tail(x, y, n, gid, gstride, a, b);
    s.finish(sr_out, srx_out, sr2_out);
}

// Single-launch variant: pass1 + in-launch combine by the LAST-arriving
// block (agent-scope release/acquire per cdna_hip_programming.md §6 G16;
// saves the finish launch + its ~4.4 us single-block latency).  The ticket
// counter is MONOTONIC: last-of-this-call iff old % gridDim == gridDim-1,
// so no per-call zeroing is needed (grid is a power of two -> the u32 wrap
// stays consistent).  One workspace+ticket per model instance; calls on one
// stream serialize, so slab reuse across calls is safe.
template <typename T>
__global__ __launch_bounds__(256) void k_gaussian_linear_fused(
    const T* __restrict__ x,
    const T* __restrict__ y,
    long long n,
    double a_d,
    double b_d,
    double inv_sig2,
    double logp_const,
    double* __restrict__ slab,       // [gridDim][3]
    unsigned* __restrict__ ticket,   // monotonic arrival counter
    double* __restrict__ out3,       // device result
    double* __restrict__ out3_host,  // mapped pinned mailbox (nullable)
    unsigned long long seq,          // call sequence for the mailbox flag
    const double* __restrict__ theta_dev  // optional [a, b] device buffer
) {
    using TR = VecTraits<T>;
    using A = typename TR::acc_t;
    constexpr int VEC = TR::VEC;
    // theta from device memory enables hipGraph replay with varying theta
    const double a = theta_dev ? theta_dev[0] : a_d;
    const double b = theta_dev ? theta_dev[1] : b_d;

    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long gstride = (long long)gridDim.x * blockDim.x;

    double sr, srx, sr2;
    gauss_accumulate<T>(x, y, n, gid, gstride, a, b, sr, srx, sr2);

    __shared__ double lds[4 * 3 + 1];  // ONE shared object (reduce + flag)
    double acc[3] = {sr2, sr, srx};
    block_reduce_add<3>(acc, lds);
    if (threadIdx.x == 0) {
        double* s = slab + 3 * (long long)blockIdx.x;
        // write-through publish: sc1 stores leave L2 immediately; drain this
        // wave's stores before the ticket so the count never overtakes them
        store_sc1_f64(&s[0], acc[0]);
        store_sc1_f64(&s[1], acc[1]);
        store_sc1_f64(&s[2], acc[2]);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        // Sharded arrival tickets (one word saturates at ~88 atomics/us ->
        // 2048 arrivals ~ 23 us measured; 8 group words on separate cache
        // lines + a top word cut that ~8x).  Grouping is by blockIdx
        // parity -- a pure partition, no XCD-placement assumption.
        const unsigned ngroups = gridDim.x < 8 ? gridDim.x : 8;
        const unsigned gsize = gridDim.x / ngroups;
        const unsigned grp = blockIdx.x % ngroups;
        bool last = false;
        const unsigned old = __hip_atomic_fetch_add(
            (gu32_t*)(ticket + 16 * grp), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old % gsize == gsize - 1) {  // last arrival of this group
            const unsigned t = __hip_atomic_fetch_add(
                (gu32_t*)(ticket + 16 * 8), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            last = (t % ngroups) == (ngroups - 1);
        }
        lds[12] = last ? 1.0 : 0.0;
    }
    __syncthreads();
    if (lds[12] == 0.0) return;

    // last-arriving block: reduce every block's slab entry with sc1 loads
    // (L1-bypassing; matches the sc1-stored data, no acquire fence needed)
    double fin[3] = {0.0, 0.0, 0.0};
    for (unsigned i = threadIdx.x; i < gridDim.x; i += blockDim.x) {
#pragma unroll
        for (int k = 0; k < 3; ++k) fin[k] += load_sc1_f64(&slab[3 * (long long)i + k]);
    }
    __syncthreads();  // lds[0..11] reused below
    block_reduce_add<3>(fin, lds);
    if (threadIdx.x == 0) {
        const double v0 = logp_const - 0.5 * inv_sig2 * fin[0];
        const double v1 = inv_sig2 * fin[1];
        const double v2 = inv_sig2 * fin[2];
        out3[0] = v0;
        out3[1] = v1;
        out3[2] = v2;
        if (out3_host != nullptr) {
            out3_host[0] = v0;
            out3_host[1] = v1;
            out3_host[2] = v2;
            __threadfence_system();  // results visible to host before the flag
            ((unsigned long long*)out3_host)[3] = seq;
        }
    }
}

// ---------------------------------------------------------------------------
// C entry points (ctypes-friendly; orchestration incl. zeroing + launches)
// ---------------------------------------------------------------------------

extern "C" {

const char* fed_last_hip_error(void) { return hipGetErrorString(hipGetLastError()); }

// workspace layout (fp64 words): [0..72) = 9 ticket words, 64 B apart
// (8 groups + 1 top; MUST be zero-initialized once), [72..72+3*grid) =
// fp64 partial slab.  ws_bytes >= (72 + 3*grid_max) * 8.
static int gaussian_linear_impl(
    const void* x, const void* y, long long n,
    double a, double b, double sigma,
    double* out3, double* out3_host,
    double* workspace, long long ws_bytes,
    int dtype, hipStream_t stream, unsigned long long seq,
    const double* theta_dev = nullptr
) {
    const double inv_sig2 = 1.0 / (sigma * sigma);
    const double logp_const = -0.5 * (double)n * log(2.0 * M_PI * sigma * sigma);
    const int block = 256;
    int grid;
    switch (dtype) {
        case FED_F32: grid = pick_grid(n / 4, block); break;
        case FED_F64: grid = pick_grid(n / 2, block); break;
        case FED_BF16: grid = pick_grid(n / 8, block); break;
        default: return -2;
    }
    long long ws_cap = (ws_bytes / 8 - 72) / 3;
    if (grid > ws_cap) grid = (int)ws_cap;
    if (grid < 1) return -3;
    // power of two so the monotonic u32 tickets wrap consistently
    while (grid & (grid - 1)) grid &= grid - 1;
    unsigned* ticket = (unsigned*)workspace;  // 9 words, 64 B apart
    double* slab = workspace + 72;
    switch (dtype) {
        case FED_F32:
            hipLaunchKernelGGL(k_gaussian_linear_fused<float>, dim3(grid), dim3(block), 0, stream,
                               (const float*)x, (const float*)y, n, a, b, inv_sig2, logp_const,
                               slab, ticket, out3, out3_host, seq, theta_dev);
            break;
        case FED_F64:
            hipLaunchKernelGGL(k_gaussian_linear_fused<double>, dim3(grid), dim3(block), 0, stream,
                               (const double*)x, (const double*)y, n, a, b, inv_sig2, logp_const,
                               slab, ticket, out3, out3_host, seq, theta_dev);
            break;
        case FED_BF16:
            hipLaunchKernelGGL(k_gaussian_linear_fused<bf16_tag>, dim3(grid), dim3(block), 0, stream,
                               (const bf16_tag*)x, (const bf16_tag*)y, n, a, b, inv_sig2, logp_const,
                               slab, ticket, out3, out3_host, seq, theta_dev);
            break;
    }
    return (int)hipGetLastError();
}

int fed_gaussian_linear(
    const void* x, const void* y, long long n,
    double a, double b, double sigma,
    double* out3, double* workspace, long long ws_bytes,
    int dtype, void* stream_v
) {
    return gaussian_linear_impl(x, y, n, a, b, sigma, out3, nullptr,
                                workspace, ws_bytes, dtype, (hipStream_t)stream_v, 0);
}

// Synchronous single-call evaluation: ONE launch; the last-arriving block
// writes {logp, ga, gb, seq} into the mapped pinned mailbox; the host
// spin-reads the seq flag (no hipStreamSynchronize on the happy path).
int fed_gaussian_linear_eval(
    const void* x, const void* y, long long n,
    double a, double b, double sigma,
    double* out3_dev, double* out3_host,
    double* workspace, long long ws_bytes,
    int dtype, void* stream_v, unsigned long long seq
) {
    hipStream_t stream = (hipStream_t)stream_v;
    void* mailbox_dev = nullptr;  // device-side alias of the pinned mailbox
    hipError_t perr = hipHostGetDevicePointer(&mailbox_dev, out3_host, 0);
    if (perr != hipSuccess) return (int)perr;
    int rc = gaussian_linear_impl(x, y, n, a, b, sigma, out3_dev,
                                  (double*)mailbox_dev, workspace, ws_bytes,
                                  dtype, stream, seq);
    if (rc != 0) return rc;
    volatile unsigned long long* flag = ((volatile unsigned long long*)out3_host) + 3;
    for (long long spins = 0; spins < 400000000LL; ++spins) {  // ~>1 s bound
        if (*flag == seq) return 0;
    }
    // flag never arrived: drain the stream and surface the real error
    hipError_t serr = hipStreamSynchronize(stream);
    if (serr != hipSuccess) return (int)serr;
    return (*flag == seq) ? 0 : -5;
}

// Mapped pinned host memory for the GPU-written result mailbox.
void* fed_host_alloc(long long bytes) {
    void* p = nullptr;
    if (hipHostMalloc(&p, bytes, hipHostMallocMapped) != hipSuccess) return nullptr;
    return p;
}

int fed_host_get_device_ptr(void* host_ptr, void** dev_ptr) {
    return (int)hipHostGetDevicePointer(dev_ptr, host_ptr, 0);
}

}  // extern "C"


// Publish a small fp64 result vector to the pinned mailbox with a
// self-incrementing epoch flag -- replayable from a hipGraph (the epoch
// lives in device memory, not in baked kernel args).
__global__ __launch_bounds__(64) void k_publish_result(
    const double* __restrict__ buf, int n,
    double* __restrict__ mailbox,            // [n results][1 seq slot]
    unsigned long long* __restrict__ epoch
) {
    if (threadIdx.x == 0) {
        for (int k = 0; k < n; ++k) mailbox[k] = buf[k];
        const unsigned long long e = *epoch + 1;
        *epoch = e;
        __threadfence_system();
        ((unsigned long long*)mailbox)[n] = e;
    }
}

extern "C" int fed_publish_result(
    const double* buf, int n, double* mailbox_host,
    unsigned long long* epoch_dev, void* stream_v
) {
    void* mailbox_dev = nullptr;
    hipError_t perr = hipHostGetDevicePointer(&mailbox_dev, mailbox_host, 0);
    if (perr != hipSuccess) return (int)perr;
    hipLaunchKernelGGL(k_publish_result, dim3(1), dim3(64), 0,
                       (hipStream_t)stream_v, buf, n, (double*)mailbox_dev, epoch_dev);
    return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------
// Native multi-shard linear engine: N shards on one GPU, one call per eval
// ---------------------------------------------------------------------------
//
// The native successor of the reference's ParallelAsyncOp fan-out
// (reference op_async.py:107-132): N federated shards resident on one
// MI355X evaluate CONCURRENTLY, each on its own HIP stream; a combine
// kernel (gated by per-shard events) sums the per-shard [logp, ga, gb]
// and writes the total to the device buffer + pinned mailbox.  The whole
// fan-out costs ONE host call; the host polls the mailbox seq flag.

__global__ __launch_bounds__(64) void k_sum_shards3(
    const double* __restrict__ shard_out,  // [n_shards][3]
    int n_shards,
    double* __restrict__ out3,
    double* __restrict__ out3_host,
    unsigned long long seq
) {
    if (threadIdx.x == 0) {
        double v[3] = {0.0, 0.0, 0.0};
        for (int s = 0; s < n_shards; ++s)
            for (int k = 0; k < 3; ++k) v[k] += shard_out[3 * s + k];
        out3[0] = v[0]; out3[1] = v[1]; out3[2] = v[2];
        if (out3_host != nullptr) {
            out3_host[0] = v[0]; out3_host[1] = v[1]; out3_host[2] = v[2];
            __threadfence_system();
            ((unsigned long long*)out3_host)[3] = seq;
        }
    }
}

#define FED_MAX_SHARDS 64

struct FedLinearEngine {
    int n_shards;
    int dtype;
    double sigma;
    const void* xs[FED_MAX_SHARDS];
    const void* ys[FED_MAX_SHARDS];
    long long ns[FED_MAX_SHARDS];
    hipStream_t streams[FED_MAX_SHARDS];
    hipEvent_t events[FED_MAX_SHARDS];
    double* ws[FED_MAX_SHARDS];      // per-shard ticket+slab workspace
    double* shard_out;               // [n_shards][3] device
    double* out3;                    // device total
    double* mailbox;                 // pinned mapped {3 results, seq}
    double* mailbox_dev;
    unsigned long long seq;
};

extern "C" {

int fed_linear_engine_destroy(void* handle);

// hipGraph-capturable launch: theta read from a device buffer at kernel
// execution time (so a captured graph replays with updated theta).
int fed_gaussian_linear_theta(
    const void* x, const void* y, long long n,
    const double* theta_dev, double sigma,
    double* out3, double* workspace, long long ws_bytes,
    int dtype, void* stream_v
) {
    return gaussian_linear_impl(x, y, n, 0.0, 0.0, sigma, out3, nullptr,
                                workspace, ws_bytes, dtype, (hipStream_t)stream_v,
                                0, theta_dev);
}

void* fed_linear_engine_create(
    int n_shards, const void** xs, const void** ys, const long long* ns,
    double sigma, int dtype
) {
    if (n_shards < 1 || n_shards > FED_MAX_SHARDS) return nullptr;
    FedLinearEngine* e = new FedLinearEngine();
    e->n_shards = n_shards;
    e->dtype = dtype;
    e->sigma = sigma;
    e->seq = 0;
    const long long ws_words = 72 + 3 * 2048;
    for (int s = 0; s < n_shards; ++s) {
        e->xs[s] = xs[s];
        e->ys[s] = ys[s];
        e->ns[s] = ns[s];
        if (hipStreamCreateWithFlags(&e->streams[s], hipStreamNonBlocking) != hipSuccess ||
            hipEventCreateWithFlags(&e->events[s], hipEventDisableTiming) != hipSuccess ||
            hipMalloc(&e->ws[s], ws_words * 8) != hipSuccess ||
            hipMemset(e->ws[s], 0, ws_words * 8) != hipSuccess) {
            fed_linear_engine_destroy(e);
            return nullptr;
        }
    }
    if (hipMalloc(&e->shard_out, n_shards * 3 * 8) != hipSuccess ||
        hipMalloc(&e->out3, 3 * 8) != hipSuccess ||
        hipHostMalloc((void**)&e->mailbox, 4 * 8, hipHostMallocMapped) != hipSuccess ||
        hipHostGetDevicePointer((void**)&e->mailbox_dev, e->mailbox, 0) != hipSuccess) {
        fed_linear_engine_destroy(e);
        return nullptr;
    }
    e->mailbox[3] = 0.0;
    return e;
}

// One federated fan-out evaluation; blocks until the summed [logp, ga, gb]
// is in out3_host_result.  sync_stream (torch current stream) is made to
// wait for the combine so subsequent torch work stays ordered.
int fed_linear_engine_eval(
    void* handle, double a, double b, double* out3_host_result, void* sync_stream
) {
    FedLinearEngine* e = (FedLinearEngine*)handle;
    e->seq += 1;
    for (int s = 0; s < e->n_shards; ++s) {
        int rc = gaussian_linear_impl(
            e->xs[s], e->ys[s], e->ns[s], a, b, e->sigma,
            e->shard_out + 3 * s, nullptr,
            e->ws[s], (72 + 3 * 2048) * 8, e->dtype, e->streams[s], 0);
        if (rc != 0) return rc;
        if (hipEventRecord(e->events[s], e->streams[s]) != hipSuccess) return -7;
    }
    for (int s = 1; s < e->n_shards; ++s)
        if (hipStreamWaitEvent(e->streams[0], e->events[s], 0) != hipSuccess) return -8;
    hipLaunchKernelGGL(k_sum_shards3, dim3(1), dim3(64), 0, e->streams[0],
                       e->shard_out, e->n_shards, e->out3, e->mailbox_dev, e->seq);
    hipError_t kerr = hipGetLastError();
    if (kerr != hipSuccess) return (int)kerr;
    if (sync_stream != nullptr) {
        if (hipEventRecord(e->events[0], e->streams[0]) != hipSuccess) return -7;
        if (hipStreamWaitEvent((hipStream_t)sync_stream, e->events[0], 0) != hipSuccess)
            return -8;
    }
    volatile unsigned long long* flag = ((volatile unsigned long long*)e->mailbox) + 3;
    for (long long spins = 0; spins < 400000000LL; ++spins) {
        if (*flag == e->seq) {
            out3_host_result[0] = e->mailbox[0];
            out3_host_result[1] = e->mailbox[1];
            out3_host_result[2] = e->mailbox[2];
            return 0;
        }
    }
    hipError_t serr = hipStreamSynchronize(e->streams[0]);
    if (serr != hipSuccess) return (int)serr;
    if (*flag != e->seq) return -5;
    out3_host_result[0] = e->mailbox[0];
    out3_host_result[1] = e->mailbox[1];
    out3_host_result[2] = e->mailbox[2];
    return 0;
}

int fed_linear_engine_destroy(void* handle) {
    FedLinearEngine* e = (FedLinearEngine*)handle;
    for (int s = 0; s < e->n_shards; ++s) {
        if (e->ws[s]) (void)hipFree(e->ws[s]);
        if (e->streams[s]) (void)hipStreamDestroy(e->streams[s]);
        if (e->events[s]) (void)hipEventDestroy(e->events[s]);
    }
    if (e->shard_out) (void)hipFree(e->shard_out);
    if (e->out3) (void)hipFree(e->out3);
    if (e->mailbox) (void)hipHostFree(e->mailbox);
    delete e;
    return 0;
}

}  // extern "C"

// ---------------------------------------------------------------------------
// Device-buffer IPC plumbing for the on-node device codec (npproto.device)
// ---------------------------------------------------------------------------
// Replaces the host-copy wire path for same-node processes: arrays move
// HBM->HBM through dmabuf IPC handles (HSA_ENABLE_IPC_MODE_LEGACY=0)
// instead of D2H -> protobuf -> H2D.  ("HIP device-buffer
// codec ... device pointer or IPC handle", replacing npproto/utils.py:9-24's
// bytes() host copy.)

extern "C" {

void* fed_device_alloc(long long bytes) {
    void* p = nullptr;
    if (hipMalloc(&p, bytes) != hipSuccess) return nullptr;
    return p;
}

int fed_device_free(void* p) { return (int)hipFree(p); }

int fed_d2d_copy(void* dst, const void* src, long long bytes, void* stream_v) {
    return (int)hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice,
                               (hipStream_t)stream_v);
}

int fed_h2d_copy(void* dst, const void* src, long long bytes, void* stream_v) {
    return (int)hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice,
                               (hipStream_t)stream_v);
}

int fed_stream_sync(void* stream_v) {
    return (int)hipStreamSynchronize((hipStream_t)stream_v);
}

int fed_ipc_get_handle(void* dev_ptr, unsigned char* handle64) {
    hipIpcMemHandle_t h;
    hipError_t err = hipIpcGetMemHandle(&h, dev_ptr);
    if (err != hipSuccess) return (int)err;
    __builtin_memcpy(handle64, &h, sizeof(h));
    return 0;
}

int fed_ipc_open(const unsigned char* handle64, void** dev_ptr) {
    hipIpcMemHandle_t h;
    __builtin_memcpy(&h, handle64, sizeof(h));
    return (int)hipIpcOpenMemHandle(dev_ptr, h, hipIpcMemLazyEnablePeerAccess);
}

int fed_ipc_close(void* dev_ptr) { return (int)hipIpcCloseMemHandle(dev_ptr); }

}  // extern "C"

// ---------------------------------------------------------------------------
// Persistent evaluation-server kernel for the gaussian linear model
// ---------------------------------------------------------------------------
//
// The per-call FIXED cost of the launch-per-eval path measured ~18 us
// (launch + wave ramp + drain) against ~7 us of actual streaming at 1e7
// rows -- the boundary dominates, which is the canonical persistent-kernel
// case.  This kernel stays resident (512 blocks = 2/CU, all the resident
// shard's registers admit): block 0 polls a pinned host
// request mailbox, broadcasts {seq, theta} through device memory (sc1
// granules), every block computes its grid-stride partials, the
// last-arriver combines and publishes to the pinned result mailbox, and a
// device done-flag releases the blocks into the next iteration.
//
// RESIDENT SHARD.  The server serves one immutable shard, so each lane
// loads its first PK_CAP 16-byte vectors of x and of y ONCE, before the
// request loop, and keeps them packed in registers; per request it unpacks
// and evaluates them exactly as the streaming loop would (same elements,
// same order, same flush cadence -- results are bit-identical to streaming
// at the same grid).  Rows beyond PK_CAP vectors per lane stream from
// memory as before.  At grid 512 the 1e7-row bf16 flagship needs 10 slots
// per lane and is fully resident: a request then touches no x/y memory.
// CONTRACT: the shard is snapshotted at (re)launch -- x and y must not be
// mutated in place while the server is open.
//
// The 512 blocks must all be co-resident (every block spins on flags other
// blocks publish): __launch_bounds__(256, 2) caps the registers so 2
// blocks fit a CU, and fed_gaussian_persistent_start checks the occupancy
// query against the grid before launching.
//
// EVERY spin is bounded: on exceeding its budget a block gives up and
// exits (block 0 stamps a timeout code into the result mailbox), so the
// kernel can never hang the GPU.  The host evaluator likewise times out
// and shuts the server down.

#define PK_SENTINEL 0xFFFFFFFFFFFFFFFFull
// Spin bounds. The REQUEST poll doubles as the idle lifetime: a resident
// kernel blocks any device-wide synchronize, so it exits after ~1-2 s idle
// and the host relaunches it transparently (hipStreamQuery detects exit).
#define PK_REQ_SPIN_LIMIT 2000000ll   // ~1-2 s idle at s_sleep(8) -> self-exit
#define PK_SPIN_LIMIT 800000ll        // worker bcast poll (~1-2 s)
#define PK_DONE_SPIN_LIMIT 200000ll   // completion barrier (compute is us-scale)

struct PersistentState {       // device memory
    unsigned long long bcast_seq;   // sc1-published request broadcast
    unsigned long long done_seq;    // sc1-published completion flag
    double theta[2];
};

__device__ __forceinline__ unsigned long long load_sc1_u64(const unsigned long long* p) {
    return __hip_atomic_load((const gu64_t*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ void store_sc1_u64(unsigned long long* p, unsigned long long v) {
    __hip_atomic_store((gu64_t*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Resident 16-byte vector pairs per lane (one value for every dtype).  From
// the compiler's output for gfx950 (bf16 / f32 / f64 instantiation, VGPRs):
// 10 slots 166 / 160 / 148, 16 slots 230 / 208 / 196, 20 slots 256 / 240 /
// 228 (the bf16 one AT the 256 a lane has at 2 blocks/CU), 24 slots spill.
// 16 is the largest with margin; it holds 1.68e7 bf16 rows at grid 512 --
// the 1e7 flagship with headroom.
#define PK_CAP 16

__device__ __forceinline__ unsigned long long pk_readlane_u64(unsigned long long v, int lane) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, lane);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), lane);
    return ((unsigned long long)hi << 32) | lo;
}

// Seqlock request poll, run by the WHOLE first wave of block 0.  Layout
// [seq | a | b | seq_pre]: the host writes seq_pre, then a, b, then seq
// (release).  Lanes 0..3 each load one of the four words with ONE wave-wide
// load instruction -- one aligned 32-byte read, one host-memory round trip
// per poll -- and the words are gathered with cross-lane reads, so the
// loop's control flow is wave-uniform.  A poll that sees seq >= next AND
// seq_pre == seq has a consistent payload in hand (the mailbox is page-
// aligned, so the four words share one 64-byte line).  Quit rides seq as
// PK_SENTINEL.  Returns the accepted `next`, or PK_SENTINEL on quit or on
// exceeding the spin bound.
__device__ __forceinline__ unsigned long long pk_poll_seqlock_wave(
    const volatile double* req_host, unsigned long long next, double& a_req, double& b_req
) {
    const volatile unsigned long long* words = (const volatile unsigned long long*)req_host;
    long long spins = 0;
    while (true) {
        unsigned long long w = 0;
        if (threadIdx.x < 4) w = words[threadIdx.x];
        const unsigned long long rs = pk_readlane_u64(w, 0);
        const unsigned long long pre = pk_readlane_u64(w, 3);
        if (rs == PK_SENTINEL) return PK_SENTINEL;
        if (rs >= next && pre == rs) {
            union { unsigned long long u; double d; } ca, cb;
            ca.u = pk_readlane_u64(w, 1);
            cb.u = pk_readlane_u64(w, 2);
            a_req = ca.d;
            b_req = cb.d;
            return next;
        }
        if (rs < next)  // no new request yet: back off
            __builtin_amdgcn_s_sleep(8);
        // torn read (host mid-write): immediate re-poll
        if (++spins > PK_REQ_SPIN_LIMIT) return PK_SENTINEL;
    }
}

template <typename T>
__global__ __launch_bounds__(256, 2) void k_gaussian_persistent(
    const T* __restrict__ x,
    const T* __restrict__ y,
    long long n,
    double inv_sig2,
    double logp_const,
    double* __restrict__ slab,          // [grid][3] (ws)
    unsigned* __restrict__ ticket,      // sharded tickets (ws)
    PersistentState* __restrict__ st,   // device control block
    const volatile double* __restrict__ req_host,  // pinned seqlock: [seq | a | b | seq_pre] (seq==SENTINEL -> quit)
    double* __restrict__ res_host,      // pinned: [logp ga gb | seq]
    int seqlock_on,                     // 1: one-round-trip poll; 0: detect-then-read
    int fence_mode                      // 1: __threadfence_system publish; 0: store-drain
) {
    using TR = VecTraits<T>;
    using A = typename TR::acc_t;
    constexpr int VEC = TR::VEC;
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long gstride = (long long)gridDim.x * blockDim.x;
    const long long nvec = n / VEC;
    __shared__ double lds[4 * 3 + 4];  // reduce scratch + {seq, a, b} bcast

    // ---- snapshot this lane's resident slice (once per launch) ----------
    // Slot k holds vector gid + k*gstride of x and of y, packed as loaded.
    // The live slots are a prefix, so "slot k is live" is k < nres in the
    // load phase and in the compute phase alike; dead slots are never
    // accumulated (a zero row would add -a to the residual sum).
    int nres = 0;
#pragma unroll
    for (int k = 0; k < PK_CAP; ++k) nres += (gid + k * gstride < nvec) ? 1 : 0;
    u32x4_t rx[PK_CAP], ry[PK_CAP];
#pragma unroll
    for (int k = 0; k < PK_CAP; ++k) {
        rx[k] = u32x4_t{0u, 0u, 0u, 0u};
        ry[k] = u32x4_t{0u, 0u, 0u, 0u};
        if (k < nres) {
            const long long i = gid + k * gstride;
            rx[k] = *reinterpret_cast<const u32x4_t*>(x + i * VEC);
            ry[k] = *reinterpret_cast<const u32x4_t*>(y + i * VEC);
        }
    }

#define PK_STAMP(code)     if (blockIdx.x == 0 && threadIdx.x == 0) ((volatile unsigned long long*)res_host)[4] = (code);
    unsigned long long my_seq = 0;
    PK_STAMP(1)
    while (true) {
        // ---- acquire next request --------------------------------------
        unsigned long long next = my_seq + 1;
        if (blockIdx.x == 0) {
            if (threadIdx.x < WAVE) {
                // poll the HOST mailbox: the first wave together (seqlock,
                // one read per poll that carries the payload) or its lane 0
                // alone (detect seq, then read the payload; quit rides seq
                // as PK_SENTINEL so a poll is ONE host-memory read)
                double a_req = 0.0, b_req = 0.0;
                if (seqlock_on) {
                    next = pk_poll_seqlock_wave(req_host, next, a_req, b_req);
                } else if (threadIdx.x == 0) {
                    long long spins = 0;
                    while (true) {
                        const unsigned long long rs =
                            ((const volatile unsigned long long*)req_host)[0];
                        if (rs == PK_SENTINEL) { next = PK_SENTINEL; break; }
                        if (rs >= next) break;
                        __builtin_amdgcn_s_sleep(8);
                        if (++spins > PK_REQ_SPIN_LIMIT) { next = PK_SENTINEL; break; }
                    }
                    if (next != PK_SENTINEL) {
                        a_req = req_host[1];
                        b_req = req_host[2];
                    }
                }
                if (threadIdx.x == 0) {
                    if (next != PK_SENTINEL) {
                        // sc1 payload + drained sc1 flag (G16 R1: a plain
                        // store + vmcnt drain is NOT cross-XCD visible)
                        store_sc1_f64(&st->theta[0], a_req);
                        store_sc1_f64(&st->theta[1], b_req);
                        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                        store_sc1_u64(&st->bcast_seq, next);
                        lds[12] = (double)1.0;
                        lds[13] = a_req;
                        lds[14] = b_req;
                    } else {
                        store_sc1_u64(&st->bcast_seq, PK_SENTINEL);
                        lds[12] = -1.0;
                    }
                }
            }
        } else if (threadIdx.x == 0) {
            // poll the DEVICE broadcast (one lane per block)
            long long spins = 0;
            unsigned long long bs;
            while (true) {
                bs = load_sc1_u64(&st->bcast_seq);
                if (bs >= next || bs == PK_SENTINEL) break;
                __builtin_amdgcn_s_sleep(16);
                if (++spins > PK_SPIN_LIMIT) { bs = PK_SENTINEL; break; }
            }
            if (bs == PK_SENTINEL) {
                lds[12] = -1.0;
            } else {
                lds[12] = 1.0;
                lds[13] = load_sc1_f64(&st->theta[0]);
                lds[14] = load_sc1_f64(&st->theta[1]);
            }
        }
        __syncthreads();
        if (lds[12] < 0.0) return;  // quit or spin give-up
        PK_STAMP(2)
        const double a = lds[13];
        const double b = lds[14];
        __syncthreads();  // lds reused by the reduction below
        my_seq += 1;

        // ---- compute this block's partials ------------------------------
        // resident slots from registers, then whatever did not fit streams,
        // then the scalar tail -- gauss_accumulate's order.  The empty asm
        // makes the packed words opaque once per request: without it the
        // compiler hoists the request-invariant unpack and conversions out
        // of the request loop and holds the slice UNPACKED (hundreds of
        // registers, 1 block/CU, the grid no longer co-resident).
        GaussLaneSums<T> sums;
        {
            A xv[VEC], yv[VEC];
            // (nres likewise: hoisted, its PK_CAP lane masks spill the SGPRs)
            asm volatile("" : "+v"(nres));
#pragma unroll
            for (int k = 0; k < PK_CAP; ++k) {
                asm volatile("" : "+v"(rx[k]), "+v"(ry[k]));
                if (k < nres) {
                    TR::unpack(rx[k], xv);
                    TR::unpack(ry[k], yv);
                    sums.vector(xv, yv, a, b);
                }
            }
        }
        sums.stream(x, y, nvec, gid + PK_CAP * gstride, gstride, a, b);
        sums.tail(x, y, n, gid, gstride, a, b);
        double sr, srx, sr2;
        sums.finish(sr, srx, sr2);
        PK_STAMP(3)
        double acc[3] = {sr2, sr, srx};
        block_reduce_add<3>(acc, lds);
        bool last = false;
        if (threadIdx.x == 0) {
            double* s = slab + 3 * (long long)blockIdx.x;
            store_sc1_f64(&s[0], acc[0]);
            store_sc1_f64(&s[1], acc[1]);
            store_sc1_f64(&s[2], acc[2]);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            const unsigned ngroups = gridDim.x < 8 ? gridDim.x : 8;
            const unsigned gsize = gridDim.x / ngroups;
            const unsigned grp = blockIdx.x % ngroups;
            const unsigned old = __hip_atomic_fetch_add(
                (gu32_t*)(ticket + 16 * grp), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (old % gsize == gsize - 1) {
                const unsigned t = __hip_atomic_fetch_add(
                    (gu32_t*)(ticket + 16 * 8), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                last = (t % ngroups) == (ngroups - 1);
            }
            lds[12] = last ? 1.0 : 0.0;
        }
        __syncthreads();

        if (lds[12] != 0.0) {
            // last-arriving block: combine + publish + release the others
            double fin[3] = {0.0, 0.0, 0.0};
            for (unsigned i = threadIdx.x; i < gridDim.x; i += blockDim.x) {
#pragma unroll
                for (int k = 0; k < 3; ++k)
                    fin[k] += load_sc1_f64(&slab[3 * (long long)i + k]);
            }
            __syncthreads();
            block_reduce_add<3>(fin, lds);
            if (threadIdx.x == 0) {
                // volatile: inside the persistent loop the compiler defers /
                // elides plain mailbox stores (measured: data landed, the
                // plain u64 flag never did)
                volatile double* rh = (volatile double*)res_host;
                rh[0] = logp_const - 0.5 * inv_sig2 * fin[0];
                rh[1] = inv_sig2 * fin[1];
                rh[2] = inv_sig2 * fin[2];
                if (fence_mode) {
                    __threadfence_system();
                } else {
                    // store-drain instead of the system fence: same-box A/B
                    // measured 55.4-55.8k vs 54.7-55.7k calls/s -- ~1%,
                    // within rep noise, so the formally correct
                    // __threadfence_system stays the default and this
                    // path is kept only as the documented experiment
                    // (FED_PK_FENCE=0)
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                }
                ((volatile unsigned long long*)res_host)[3] = my_seq;
                store_sc1_u64(&st->done_seq, my_seq);
            }
        }
        PK_STAMP(4)
        // ---- completion barrier (slab must not be reused early) ---------
        if (threadIdx.x == 0) {
            long long spins = 0;
            while (load_sc1_u64(&st->done_seq) < my_seq) {
                __builtin_amdgcn_s_sleep(8);
                if (++spins > PK_DONE_SPIN_LIMIT) { lds[12] = -1.0; break; }
            }
        }
        __syncthreads();
        if (lds[12] < 0.0) return;
    }
}

struct FedPersistentLinear {
    double* ws = nullptr;          // tickets + slab
    PersistentState* st = nullptr;
    double* req = nullptr;         // pinned [seq a b seq_pre]
    double* res = nullptr;         // pinned [3 results | seq]
    hipStream_t stream = nullptr;
    unsigned long long seq = 0;
    int grid = 512;
    // launch parameters (for transparent relaunch after idle self-exit)
    const void* x = nullptr;
    const void* y = nullptr;
    long long n = 0;
    double inv_sig2 = 0;
    double logp_const = 0;
    int dtype = FED_BF16;
    void* req_dev = nullptr;
    void* res_dev = nullptr;
};

// Frees everything start allocated (a null member was never allocated).
static void persistent_free(FedPersistentLinear* e) {
    if (e->ws) (void)hipFree(e->ws);
    if (e->st) (void)hipFree(e->st);
    if (e->req) (void)hipHostFree(e->req);
    if (e->res) (void)hipHostFree(e->res);
    if (e->stream) (void)hipStreamDestroy(e->stream);
    delete e;
}

// Every block spins on flags that other blocks publish, so the whole grid
// must be resident at once.  True iff the occupancy query for this dtype's
// instantiation admits e->grid blocks on the current device.
static bool persistent_grid_fits(const FedPersistentLinear* e) {
    int per_cu = 0, dev = 0, cus = 0;
    hipError_t err;
    switch (e->dtype) {
        case FED_BF16:
            err = hipOccupancyMaxActiveBlocksPerMultiprocessor(
                &per_cu, k_gaussian_persistent<bf16_tag>, 256, 0);
            break;
        case FED_F32:
            err = hipOccupancyMaxActiveBlocksPerMultiprocessor(
                &per_cu, k_gaussian_persistent<float>, 256, 0);
            break;
        case FED_F64:
            err = hipOccupancyMaxActiveBlocksPerMultiprocessor(
                &per_cu, k_gaussian_persistent<double>, 256, 0);
            break;
        default:
            return false;
    }
    if (err != hipSuccess || hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
        return false;
    return (long long)per_cu * cus >= e->grid;
}

static int persistent_launch(FedPersistentLinear* e) {
    unsigned* ticket = (unsigned*)e->ws;
    double* slab = e->ws + 72;
    // Poll protocol A/B on top of the resident shard (same box, 5 reps
    // each, interleaved, default bench arguments): the wave-wide seqlock
    // poll 70.6-75.6k calls/s vs detect-then-read 60.4-64.3k -- one
    // 32-byte read per poll that already carries the payload saves the
    // dependent second host-memory round trip.  (The first seqlock reader
    // lost this A/B: its four volatile loads from ONE lane went out as four
    // serialized fabric transactions per poll.)  Default is therefore the
    // seqlock poll; FED_PK_SEQLOCK=0 selects the two-step poll.
    const char* sl = getenv("FED_PK_SEQLOCK");
    const int seqlock_on = sl ? (atoi(sl) != 0) : 1;
    const char* fm = getenv("FED_PK_FENCE");
    const int fence_mode = fm ? (atoi(fm) != 0) : 1;
    switch (e->dtype) {
        case FED_BF16:
            hipLaunchKernelGGL(k_gaussian_persistent<bf16_tag>, dim3(e->grid), dim3(256), 0,
                               e->stream, (const bf16_tag*)e->x, (const bf16_tag*)e->y, e->n,
                               e->inv_sig2, e->logp_const, slab, ticket, e->st,
                               (const volatile double*)e->req_dev, (double*)e->res_dev,
                               seqlock_on, fence_mode);
            break;
        case FED_F32:
            hipLaunchKernelGGL(k_gaussian_persistent<float>, dim3(e->grid), dim3(256), 0,
                               e->stream, (const float*)e->x, (const float*)e->y, e->n,
                               e->inv_sig2, e->logp_const, slab, ticket, e->st,
                               (const volatile double*)e->req_dev, (double*)e->res_dev,
                               seqlock_on, fence_mode);
            break;
        case FED_F64:
            hipLaunchKernelGGL(k_gaussian_persistent<double>, dim3(e->grid), dim3(256), 0,
                               e->stream, (const double*)e->x, (const double*)e->y, e->n,
                               e->inv_sig2, e->logp_const, slab, ticket, e->st,
                               (const volatile double*)e->req_dev, (double*)e->res_dev,
                               seqlock_on, fence_mode);
            break;
        default:
            return -2;
    }
    return (int)hipGetLastError();
}

extern "C" {

void* fed_gaussian_persistent_start(
    const void* x, const void* y, long long n, double sigma, int dtype
) {
    FedPersistentLinear* e = new FedPersistentLinear();
    {
        const char* env = getenv("FED_PERSIST_GRID");
        if (env) {
            int g = atoi(env);
            if (g >= 8 && g <= 1024 && (g & (g - 1)) == 0) e->grid = g;
        }
    }
    const long long ws_words = 72 + 3 * (long long)e->grid;
    if (hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking) != hipSuccess ||
        hipMalloc(&e->ws, ws_words * 8) != hipSuccess ||
        hipMemset(e->ws, 0, ws_words * 8) != hipSuccess ||
        hipMalloc(&e->st, sizeof(PersistentState)) != hipSuccess ||
        hipMemset(e->st, 0, sizeof(PersistentState)) != hipSuccess ||
        hipHostMalloc((void**)&e->req, 8 * 8, hipHostMallocMapped) != hipSuccess ||
        hipHostMalloc((void**)&e->res, 8 * 8, hipHostMallocMapped) != hipSuccess) {
        persistent_free(e);
        return nullptr;
    }
    for (int i = 0; i < 8; ++i) {
        e->req[i] = 0.0;
        e->res[i] = 0.0;
    }
    void* req_dev = nullptr;
    void* res_dev = nullptr;
    if (hipHostGetDevicePointer(&req_dev, e->req, 0) != hipSuccess ||
        hipHostGetDevicePointer(&res_dev, e->res, 0) != hipSuccess) {
        persistent_free(e);
        return nullptr;
    }
    e->x = x;
    e->y = y;
    e->n = n;
    e->dtype = dtype;
    e->inv_sig2 = 1.0 / (sigma * sigma);
    e->logp_const = -0.5 * (double)n * log(2.0 * M_PI * sigma * sigma);
    e->req_dev = req_dev;
    e->res_dev = res_dev;
    if (!persistent_grid_fits(e) || persistent_launch(e) != 0) {
        persistent_free(e);
        return nullptr;
    }
    return e;
}

int fed_gaussian_persistent_eval(void* handle, double a, double b, double* out3) {
    FedPersistentLinear* e = (FedPersistentLinear*)handle;
    e->seq += 1;
    __atomic_store_n((unsigned long long*)&e->req[3], e->seq, __ATOMIC_RELEASE);
    e->req[1] = a;
    e->req[2] = b;
    __atomic_store_n((unsigned long long*)&e->req[0], e->seq, __ATOMIC_RELEASE);
    volatile unsigned long long* flag = ((volatile unsigned long long*)e->res) + 3;
    int relaunches = 0;
    for (long long spins = 0; spins < 4000000000LL; ++spins) {
        if (*flag >= e->seq) {
            out3[0] = e->res[0];
            out3[1] = e->res[1];
            out3[2] = e->res[2];
            return 0;
        }
        if ((spins & 0xFFFFF) == 0xFFFFF) {  // every ~1M spins (~1-2 ms)
            // server may have idle-exited (bounded request poll); relaunch --
            // the fresh kernel sees the pending req_seq and serves it
            if (hipStreamQuery(e->stream) != hipErrorNotReady) {
                if (relaunches++ > 4) return -6;
                if (persistent_launch(e) != 0) return -7;
            }
        }
    }
    return -6;
}

int fed_gaussian_persistent_debug(void* handle, double* req8, double* res8) {
    FedPersistentLinear* e = (FedPersistentLinear*)handle;
    for (int i = 0; i < 8; ++i) {
        req8[i] = e->req[i];
        res8[i] = e->res[i];
    }
    return 0;
}

int fed_gaussian_persistent_stop(void* handle) {
    FedPersistentLinear* e = (FedPersistentLinear*)handle;
    __atomic_store_n((unsigned long long*)&e->req[0], PK_SENTINEL, __ATOMIC_RELEASE);
    hipError_t err = hipStreamSynchronize(e->stream);  // kernel exits on quit
    persistent_free(e);
    return (int)err;
}

}  // extern "C"
