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
// shard's registers admit) and serves one request per loop iteration.
//
// PROTOCOL.  Every hand-off is a set of 8-byte GRANULES {tag << 32 | 32-bit
// value}, tag = low 32 bits of the call's sequence number, each written by
// ONE aligned 8-byte agent-scope store from a lane and read by a relaxed
// agent-scope load: the data is the flag.  There is no separate flag word, no
// store drain, no fence, no atomic read-modify-write.  A 64-bit value is two
// granules; a reader accepts a value only when the tags of ALL its own
// granules equal the call's tag, never on a neighbour's.
//   1. request    host -> block 0: pinned [seq | a | b | seq_pre] seqlock,
//                 polled by block 0's first wave (FED_PK_SEQLOCK=0: lane 0
//                 detects seq, then reads a, b).
//   2. broadcast  block 0 -> all: ONE 64-byte line of five granules {a lo,
//                 a hi, b lo, b hi, control (0 serve, 1 quit)}, stored by
//                 lanes 0..4 of one wave with one store instruction; every
//                 other block's first wave polls it with one wave-wide load.
//   3. compute    from the register-resident shard (below).
//   4. partials   every block (block 0 too) -> its own 64-byte slot: three
//                 f64 block sums as six granules, one store instruction.
//   5. combine    block 0 is the FIXED combiner: thread t owns the slots of
//                 blocks t, t+256, ..., re-reads those whose six tags are not
//                 yet all current, and adds them in increasing block index
//                 from 0.0; then the block reduction -- the summation order
//                 of the former last-arriver combine, so results are
//                 bit-identical to it.
//   6. publish    block 0 -> host: [logp, ga, gb] as six granules plus a
//                 seventh {tag, code} word in one 64-byte pinned line, one
//                 store instruction; the host spins until all six tags are
//                 its sequence's.  code != 0 under the awaited tag means the
//                 server gave up (1 idle exit or quit, 2 combine timeout).
//
// WHY NO COMPLETION BARRIER.  Slot and line reuse is ordered by causality:
//   - a worker stores call s+1's granules only after it has seen broadcast
//     s+1;
//   - block 0 issues broadcast s+1 only after the host has sent request s+1;
//   - the host sends request s+1 only after it has received result s;
//   - block 0 publishes result s only after its sweep of call s is complete,
//     i.e. after it has read every slot of call s, each of which was stored
//     by a block that had read broadcast s.
// So nobody overwrites a granule that a reader of the previous call still
// needs, and a reader can only ever see "previous call" or "this call".
//
// INIT INVARIANT.  In the steady state every tag in the three tagged areas
// (broadcast line, partial slots, result line) names the previous call.
// The host establishes exactly that before every (re)launch: a small kernel
// on the server's stream sets every tag to the low 32 bits of the last
// served sequence, and the server starts counting from that sequence
// (kernel argument).  Tags are compared for equality only, so the 32-bit
// wrap is harmless, and a relaunched server can never take a granule left
// by the exited one for current.  Zeroing would not do: 0 is a valid tag
// once per 2^32 calls.
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
// The 512 blocks must all be co-resident (every block spins on words other
// blocks publish): __launch_bounds__(256, 2) caps the registers so 2
// blocks fit a CU, and fed_gaussian_persistent_start checks the occupancy
// query against the grid before launching.
//
// EVERY spin is bounded, in ticks of the constant-rate clock (100 MHz)
// sampled every PK_CLOCK_EVERY polls, and the bounds are ORDERED so that
// block 0 always decides: its request poll (the idle lifetime) and its
// combine sweep are far shorter than the workers' broadcast poll, and on
// either give-up block 0 broadcasts the quit control word, which releases
// every worker at once.  A worker's own bound only matters if block 0 is
// gone without a word.  The host evaluator likewise times out and shuts
// the server down.

#define PK_SENTINEL 0xFFFFFFFFFFFFFFFFull
// A resident kernel blocks any device-wide synchronize, so the request poll
// doubles as the idle lifetime: block 0 exits after PK_IDLE_TICKS without a
// request and the host relaunches the server transparently.
#define PK_TICKS_PER_MS 100000ll                  // wall_clock64(): 100 MHz
#define PK_IDLE_TICKS (1500 * PK_TICKS_PER_MS)    // block 0 request poll: 1.5 s
#define PK_SWEEP_TICKS (250 * PK_TICKS_PER_MS)    // combine sweep: 0.25 s (compute is us-scale)
#define PK_BCAST_TICKS (6000 * PK_TICKS_PER_MS)   // workers: 6 s > 3x (idle + sweep)
#define PK_CLOCK_EVERY 256                        // polls between clock samples
// s_sleep quantum of the workers' broadcast poll (A/B in profiles/PROFILES.md)
#ifndef PK_BCAST_SLEEP
#define PK_BCAST_SLEEP 16
#endif

// control block (device memory, 64-bit words): [0..8) the broadcast line,
// then one 8-word (64-byte) partial slot per block
#define PK_CTL_SLOT0 8
#define PK_CTL_WORDS(grid) (8 + 8 * (long long)(grid))

__device__ __forceinline__ unsigned long long load_sc1_u64(const unsigned long long* p) {
    return __hip_atomic_load((const gu64_t*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ void store_sc1_u64(unsigned long long* p, unsigned long long v) {
    __hip_atomic_store((gu64_t*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the pinned result line is read by the host: same form, system scope
__device__ __forceinline__ void store_sys_u64(unsigned long long* p, unsigned long long v) {
    __hip_atomic_store((gu64_t*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

__device__ __forceinline__ unsigned long long pk_granule(unsigned tag, unsigned value) {
    return ((unsigned long long)tag << 32) | value;
}

__device__ __forceinline__ unsigned long long pk_f64_bits(double d) {
    union { double d; unsigned long long u; } c;
    c.d = d;
    return c.u;
}

__device__ __forceinline__ double pk_f64_from_halves(unsigned long long lo, unsigned long long hi) {
    union { unsigned long long u; double d; } c;
    c.u = (hi << 32) | (lo & 0xFFFFFFFFull);
    return c.d;
}

// 32-bit half `lane` (0..5) of three 64-bit words laid out lo, hi, lo, hi, ..
__device__ __forceinline__ unsigned pk_half_of3(
    unsigned long long w0, unsigned long long w1, unsigned long long w2, int lane
) {
    const unsigned long long w = lane < 2 ? w0 : (lane < 4 ? w1 : w2);
    return (unsigned)((lane & 1) ? (w >> 32) : w);
}

// Stage timing (profiling build only, -DFED_PK_PROF): lane 0 of every block
// stamps the constant-rate clock into its 8-word slot of a device buffer;
// the slot always describes the last served call.  Slots: 0 request
// accepted / broadcast seen, 1 compute done, 2 partial stored, 3 combine
// done, 4 publish issued (3 and 4: the combining block only).
#ifdef FED_PK_PROF
#define PK_PROF_PARAM , unsigned long long* prof
#define PK_PROF_ARG(e) , (e)->prof
#define PK_PROF(slot) \
    store_sc1_u64(&prof[8 * (long long)blockIdx.x + (slot)], wall_clock64());
#else
#define PK_PROF_PARAM
#define PK_PROF_ARG(e)
#define PK_PROF(slot)
#endif

// Resident 16-byte vector pairs per lane (one value for every dtype).  From
// the compiler's output for gfx950 (bf16 / f32 / f64 instantiation, VGPRs):
// 10 slots 166 / 160 / 148, 16 slots 230 / 208 / 196, 20 slots 256 / 240 /
// 228 (the bf16 one AT the 256 a lane has at 2 blocks/CU), 24 slots spill.
// 16 is the largest with margin; it holds 1.68e7 bf16 rows at grid 512 --
// the 1e7 flagship with headroom.
#define PK_CAP 16

// A spin's budget in constant-rate ticks, kept off the fast path: the clock
// is read only every PK_CLOCK_EVERY polls and the first reading starts the
// budget, so a poll that succeeds early never reads it.
struct PkSpinBound {
    long long t0 = 0;
    unsigned polls = 0;
    __device__ __forceinline__ bool expired(long long budget) {
        if ((++polls % PK_CLOCK_EVERY) != 0) return false;
        const long long now = wall_clock64();
        if (t0 == 0) {
            t0 = now;
            return false;
        }
        return now - t0 > budget;
    }
};

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
// exceeding the idle lifetime.
__device__ __forceinline__ unsigned long long pk_poll_seqlock_wave(
    const volatile double* req_host, unsigned long long next, double& a_req, double& b_req
) {
    const volatile unsigned long long* words = (const volatile unsigned long long*)req_host;
    PkSpinBound bound;
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
        if (bound.expired(PK_IDLE_TICKS)) return PK_SENTINEL;
    }
}

// Sets every tag of the three tagged areas to `tag` (the last served
// sequence), values 0: the steady-state invariant, before every (re)launch.
__global__ __launch_bounds__(256) void k_persistent_init(
    unsigned long long* ctl, long long ctl_words, unsigned long long* res_host, unsigned tag
) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < ctl_words) store_sc1_u64(&ctl[i], pk_granule(tag, 0u));
    if (i < 8) store_sys_u64(&res_host[i], pk_granule(tag, 0u));
}

template <typename T>
__global__ __launch_bounds__(256, 2) void k_gaussian_persistent(
    const T* __restrict__ x,
    const T* __restrict__ y,
    long long n,
    double inv_sig2,
    double logp_const,
    unsigned long long* ctl,            // device: broadcast line + partial slots
    const volatile double* __restrict__ req_host,  // pinned seqlock: [seq | a | b | seq_pre] (seq==SENTINEL -> quit)
    unsigned long long* res_host,       // pinned result line: 6 granules + {tag, code}
    int seqlock_on,                     // 1: one-round-trip poll; 0: detect-then-read
    unsigned long long seq0             // the last sequence already served
    PK_PROF_PARAM
) {
    using TR = VecTraits<T>;
    using A = typename TR::acc_t;
    constexpr int VEC = TR::VEC;
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long gstride = (long long)gridDim.x * blockDim.x;
    const long long nvec = n / VEC;
    __shared__ double lds[4 * 3 + 4];  // reduce scratch + {go, a, b} bcast

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

    unsigned long long my_seq = seq0;
    unsigned long long* const slot = ctl + PK_CTL_SLOT0 + 8 * (long long)blockIdx.x;
    while (true) {
        // ---- acquire next request (first wave of every block) ----------
        const unsigned tag = (unsigned)(my_seq + 1);
        if (threadIdx.x < WAVE) {
            // (opaque per request, like nres below: hoisted out of the
            // request loop, the lane predicates of the granule stores and
            // loads live in SGPR pairs and spill)
            int lane = threadIdx.x;
            asm volatile("" : "+v"(lane));
            unsigned long long wa = 0, wb = 0;  // theta, as bits
            unsigned ctrl = 0;                  // 0 serve, else leave
            if (blockIdx.x == 0) {
                // poll the HOST mailbox: the wave together (seqlock, one
                // read per poll that carries the payload) or its lane 0
                // alone (detect seq, then read the payload; quit rides seq
                // as PK_SENTINEL so a poll is ONE host-memory read)
                unsigned long long next = my_seq + 1;
                double a_req = 0.0, b_req = 0.0;
                if (seqlock_on) {
                    next = pk_poll_seqlock_wave(req_host, next, a_req, b_req);
                } else {
                    if (lane == 0) {
                        PkSpinBound bound;
                        while (true) {
                            const unsigned long long rs =
                                ((const volatile unsigned long long*)req_host)[0];
                            if (rs == PK_SENTINEL) { next = PK_SENTINEL; break; }
                            if (rs >= next) break;
                            __builtin_amdgcn_s_sleep(8);
                            if (bound.expired(PK_IDLE_TICKS)) {
                                next = PK_SENTINEL;
                                break;
                            }
                        }
                        if (next != PK_SENTINEL) {
                            a_req = req_host[1];
                            b_req = req_host[2];
                        }
                    }
                    next = pk_readlane_u64(next, 0);  // lane 0's answer, wave-wide
                }
                ctrl = (next == PK_SENTINEL) ? 1u : 0u;
                wa = pk_readlane_u64(pk_f64_bits(a_req), 0);
                wb = pk_readlane_u64(pk_f64_bits(b_req), 0);
                if (lane == 0 && ctrl == 0u) { PK_PROF(0) }
                // the broadcast: five granules, one store instruction
                const unsigned v = lane < 4 ? pk_half_of3(wa, wb, 0ull, lane) : ctrl;
                if (lane < 5) store_sc1_u64(&ctl[lane], pk_granule(tag, v));
                // idle exit or quit: tell the host under the tag it would wait for
                if (ctrl != 0u && lane == 0) store_sys_u64(&res_host[6], pk_granule(tag, 1u));
            } else {
                // poll the DEVICE broadcast line: one wave-wide load, accept
                // when all five tags are this call's
                PkSpinBound bound;
                unsigned long long g = 0;
                bool seen = false;
                while (true) {
                    if (lane < 5) g = load_sc1_u64(&ctl[lane]);
                    const bool ok = lane >= 5 || (unsigned)(g >> 32) == tag;
                    if (__all(ok)) { seen = true; break; }
                    __builtin_amdgcn_s_sleep(PK_BCAST_SLEEP);
                    if (bound.expired(PK_BCAST_TICKS)) break;
                }
                const unsigned lo = (unsigned)g;
                wa = ((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)lo, 1) << 32) |
                     (unsigned)__builtin_amdgcn_readlane((int)lo, 0);
                wb = ((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)lo, 3) << 32) |
                     (unsigned)__builtin_amdgcn_readlane((int)lo, 2);
                ctrl = seen ? (unsigned)__builtin_amdgcn_readlane((int)lo, 4) : 2u;
                if (lane == 0 && ctrl == 0u) { PK_PROF(0) }
            }
            if (lane == 0) {
                lds[12] = ctrl == 0u ? 1.0 : -1.0;
                lds[15] = 0.0;  // block 0's sweep-timeout word
                lds[13] = pk_f64_from_halves(wa, wa >> 32);
                lds[14] = pk_f64_from_halves(wb, wb >> 32);
            }
        }
        __syncthreads();
        if (lds[12] < 0.0) return;  // quit, idle exit or spin give-up
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
        if (threadIdx.x == 0) { PK_PROF(1) }
        double acc[3] = {sr2, sr, srx};
        block_reduce_add<3>(acc, lds);
        // ---- partials: six granules into this block's slot ---------------
        if (threadIdx.x < WAVE) {
            int lane = threadIdx.x;
            asm volatile("" : "+v"(lane));
            const unsigned long long w0 = pk_readlane_u64(pk_f64_bits(acc[0]), 0);
            const unsigned long long w1 = pk_readlane_u64(pk_f64_bits(acc[1]), 0);
            const unsigned long long w2 = pk_readlane_u64(pk_f64_bits(acc[2]), 0);
            if (lane < 6) store_sc1_u64(&slot[lane], pk_granule(tag, pk_half_of3(w0, w1, w2, lane)));
            if (lane == 0) { PK_PROF(2) }
        }
        if (blockIdx.x != 0) continue;

        // ---- block 0: sweep the slots, combine, publish ------------------
        // Thread t owns blocks t, t+256, ...; two slots are in flight per
        // pass and only slots whose tags are not all current are re-read.
        double fin[3] = {0.0, 0.0, 0.0};
        bool timed_out = false;
        {
            PkSpinBound bound;
            for (unsigned base = threadIdx.x; base < gridDim.x; base += 2 * 256) {
                const unsigned long long* s0 = ctl + PK_CTL_SLOT0 + 8 * (long long)base;
                const unsigned long long* s1 = s0 + 8 * 256;
                const bool have1 = base + 256 < gridDim.x;
                bool p0 = true, p1 = have1;
                unsigned long long g0[6] = {0, 0, 0, 0, 0, 0}, g1[6] = {0, 0, 0, 0, 0, 0};
                while (p0 || p1) {
                    if (p0) {
#pragma unroll
                        for (int k = 0; k < 6; ++k) g0[k] = load_sc1_u64(&s0[k]);
                    }
                    if (p1) {
#pragma unroll
                        for (int k = 0; k < 6; ++k) g1[k] = load_sc1_u64(&s1[k]);
                    }
                    if (p0) {
                        bool m = true;
#pragma unroll
                        for (int k = 0; k < 6; ++k) m &= (unsigned)(g0[k] >> 32) == tag;
                        p0 = !m;
                    }
                    if (p1) {
                        bool m = true;
#pragma unroll
                        for (int k = 0; k < 6; ++k) m &= (unsigned)(g1[k] >> 32) == tag;
                        p1 = !m;
                    }
                    if (p0 || p1) {
                        __builtin_amdgcn_s_sleep(1);
                        if (bound.expired(PK_SWEEP_TICKS)) {
                            timed_out = true;
                            break;
                        }
                    }
                }
                if (timed_out) break;
#pragma unroll
                for (int k = 0; k < 3; ++k) fin[k] += pk_f64_from_halves(g0[2 * k], g0[2 * k + 1]);
                if (have1) {
#pragma unroll
                    for (int k = 0; k < 3; ++k)
                        fin[k] += pk_f64_from_halves(g1[2 * k], g1[2 * k + 1]);
                }
            }
        }
        if (timed_out) lds[15] = 1.0;
        __syncthreads();  // (also separates the two reductions' uses of lds)
        if (lds[15] != 0.0) {
            // give up: release the workers under the NEXT call's tag (the
            // one they wait for), tell the host under this call's, exit
            unsigned t = threadIdx.x;
            asm volatile("" : "+v"(t));  // keep this cold path's predicates out of the loop's SGPRs
            if (t < 5) store_sc1_u64(&ctl[t], pk_granule(tag + 1u, t == 4 ? 1u : 0u));
            if (t == 0) store_sys_u64(&res_host[6], pk_granule(tag, 2u));
            return;
        }
        block_reduce_add<3>(fin, lds);
        if (threadIdx.x < WAVE) {
            int lane = threadIdx.x;
            asm volatile("" : "+v"(lane));
            const unsigned long long w0 =
                pk_readlane_u64(pk_f64_bits(logp_const - 0.5 * inv_sig2 * fin[0]), 0);
            const unsigned long long w1 = pk_readlane_u64(pk_f64_bits(inv_sig2 * fin[1]), 0);
            const unsigned long long w2 = pk_readlane_u64(pk_f64_bits(inv_sig2 * fin[2]), 0);
            if (lane == 0) { PK_PROF(3) }
            // the result line: six granules + {tag, 0}, one store instruction
            const unsigned v = lane < 6 ? pk_half_of3(w0, w1, w2, lane) : 0u;
            if (lane < 7) store_sys_u64(&res_host[lane], pk_granule(tag, v));
            if (lane == 0) { PK_PROF(4) }
        }
    }
}

#ifdef FED_PK_PROF
#include <time.h>
static inline long long pk_host_ns(void) {
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (long long)ts.tv_sec * 1000000000ll + ts.tv_nsec;
}
#endif

struct FedPersistentLinear {
    unsigned long long* ctl = nullptr;  // broadcast line + partial slots
    double* req = nullptr;         // pinned [seq a b seq_pre]
    double* res = nullptr;         // pinned result line (8 words)
    hipStream_t stream = nullptr;
    unsigned long long seq = 0;    // last sequence sent
    int grid = 512;
    int relaunches = 0;            // launches after the first one
    // launch parameters (for transparent relaunch after idle self-exit)
    const void* x = nullptr;
    const void* y = nullptr;
    long long n = 0;
    double inv_sig2 = 0;
    double logp_const = 0;
    int dtype = FED_BF16;
    void* req_dev = nullptr;
    void* res_dev = nullptr;
#ifdef FED_PK_PROF
    unsigned long long* prof = nullptr;  // [grid][8] device stamps
    long long host_ns[2] = {0, 0};       // request written, result seen
#endif
};

// Frees everything start allocated (a null member was never allocated).
static void persistent_free(FedPersistentLinear* e) {
    if (e->ctl) (void)hipFree(e->ctl);
    if (e->req) (void)hipHostFree(e->req);
    if (e->res) (void)hipHostFree(e->res);
    if (e->stream) (void)hipStreamDestroy(e->stream);
#ifdef FED_PK_PROF
    if (e->prof) (void)hipFree(e->prof);
#endif
    delete e;
}

// Every block spins on words that other blocks publish, so the whole grid
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

// (Re)launch the server so that it continues after sequence `served`: first
// the init kernel (every tag = low 32 bits of `served`, see INIT INVARIANT),
// then the resident kernel, both on the server's stream.
static int persistent_launch(FedPersistentLinear* e, unsigned long long served) {
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
    const long long ctl_words = PK_CTL_WORDS(e->grid);
    hipLaunchKernelGGL(k_persistent_init, dim3((unsigned)((ctl_words + 255) / 256)), dim3(256), 0,
                       e->stream, e->ctl, ctl_words, (unsigned long long*)e->res_dev,
                       (unsigned)served);
    if (hipGetLastError() != hipSuccess) return -3;
    switch (e->dtype) {
        case FED_BF16:
            hipLaunchKernelGGL(k_gaussian_persistent<bf16_tag>, dim3(e->grid), dim3(256), 0,
                               e->stream, (const bf16_tag*)e->x, (const bf16_tag*)e->y, e->n,
                               e->inv_sig2, e->logp_const, e->ctl,
                               (const volatile double*)e->req_dev,
                               (unsigned long long*)e->res_dev, seqlock_on,
                               served PK_PROF_ARG(e));
            break;
        case FED_F32:
            hipLaunchKernelGGL(k_gaussian_persistent<float>, dim3(e->grid), dim3(256), 0,
                               e->stream, (const float*)e->x, (const float*)e->y, e->n,
                               e->inv_sig2, e->logp_const, e->ctl,
                               (const volatile double*)e->req_dev,
                               (unsigned long long*)e->res_dev, seqlock_on,
                               served PK_PROF_ARG(e));
            break;
        case FED_F64:
            hipLaunchKernelGGL(k_gaussian_persistent<double>, dim3(e->grid), dim3(256), 0,
                               e->stream, (const double*)e->x, (const double*)e->y, e->n,
                               e->inv_sig2, e->logp_const, e->ctl,
                               (const volatile double*)e->req_dev,
                               (unsigned long long*)e->res_dev, seqlock_on,
                               served PK_PROF_ARG(e));
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
        // initial host sequence (tests start just below the 32-bit tag wrap)
        const char* s0 = getenv("FED_PK_SEQ0");
        if (s0) e->seq = strtoull(s0, nullptr, 10);
    }
    if (hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking) != hipSuccess ||
        hipMalloc(&e->ctl, PK_CTL_WORDS(e->grid) * 8) != hipSuccess ||
        hipHostMalloc((void**)&e->req, 8 * 8, hipHostMallocMapped) != hipSuccess ||
        hipHostMalloc((void**)&e->res, 8 * 8, hipHostMallocMapped) != hipSuccess) {
        persistent_free(e);
        return nullptr;
    }
    for (int i = 0; i < 8; ++i) {
        e->req[i] = 0.0;
        e->res[i] = 0.0;
    }
    // no request pending: seq and seq_pre name the last sequence sent
    ((unsigned long long*)e->req)[0] = e->seq;
    ((unsigned long long*)e->req)[3] = e->seq;
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
#ifdef FED_PK_PROF
    if (hipMalloc(&e->prof, 8 * 8 * (long long)e->grid) != hipSuccess ||
        hipMemset(e->prof, 0, 8 * 8 * (long long)e->grid) != hipSuccess) {
        persistent_free(e);
        return nullptr;
    }
#endif
    if (!persistent_grid_fits(e) || persistent_launch(e, e->seq) != 0) {
        persistent_free(e);
        return nullptr;
    }
    return e;
}

int fed_gaussian_persistent_eval(void* handle, double a, double b, double* out3) {
    FedPersistentLinear* e = (FedPersistentLinear*)handle;
    e->seq += 1;
    const unsigned tag = (unsigned)e->seq;
#ifdef FED_PK_PROF
    e->host_ns[0] = pk_host_ns();
#endif
    __atomic_store_n((unsigned long long*)&e->req[3], e->seq, __ATOMIC_RELEASE);
    e->req[1] = a;
    e->req[2] = b;
    __atomic_store_n((unsigned long long*)&e->req[0], e->seq, __ATOMIC_RELEASE);
    // the result line: aligned 8-byte loads; a value counts only under its
    // own granules' tags
    volatile unsigned long long* line = (volatile unsigned long long*)e->res;
    int relaunches = 0;
    for (long long spins = 0; spins < 4000000000LL; ++spins) {
        unsigned long long g[6];
        bool ok = true;
        for (int k = 0; k < 6; ++k) {
            g[k] = line[k];
            ok &= (unsigned)(g[k] >> 32) == tag;
        }
        if (ok) {
#ifdef FED_PK_PROF
            e->host_ns[1] = pk_host_ns();
#endif
            for (int k = 0; k < 3; ++k) {
                union { unsigned long long u; double d; } c;
                c.u = (g[2 * k + 1] << 32) | (g[2 * k] & 0xFFFFFFFFull);
                out3[k] = c.d;
            }
            return 0;
        }
        // seventh word: the server gave up under the tag we wait for (idle
        // exit racing this request, or a combine timeout) and is exiting
        const unsigned long long code = line[6];
        const bool gave_up = (unsigned)(code >> 32) == tag && (unsigned)code != 0u;
        if (gave_up || (spins & 0xFFFFF) == 0xFFFFF) {  // or every ~1M spins (~1-2 ms)
            if (gave_up) {
                if (hipStreamSynchronize(e->stream) != hipSuccess) return -7;
                line[6] = ((unsigned long long)(tag - 1u)) << 32;  // consumed
            }
            // server may have idle-exited (bounded request poll); relaunch at
            // the last served sequence -- the fresh kernel sees the pending
            // request and serves it exactly once
            if (gave_up || hipStreamQuery(e->stream) != hipErrorNotReady) {
                if (relaunches++ > 4) return -6;
                e->relaunches += 1;
                if (persistent_launch(e, e->seq - 1) != 0) return -7;
            }
        }
    }
    return -6;
}

// launches of the server after the first one (idle exits that were followed
// by a call)
int fed_gaussian_persistent_relaunch_count(void* handle) {
    return ((FedPersistentLinear*)handle)->relaunches;
}

#ifdef FED_PK_PROF
// Copies out the stamps of the last served call ([grid][8] clock words) and
// the host's two timestamps (ns); call it while the server is idle.  The
// copy runs on a stream of its own: the resident kernel occupies e->stream.
int fed_gaussian_persistent_prof(
    void* handle, unsigned long long* stamps, long long cap_words, long long* host_ns2
) {
    FedPersistentLinear* e = (FedPersistentLinear*)handle;
    const long long words = 8 * (long long)e->grid;
    if (cap_words < words) return -2;
    hipStream_t cs = nullptr;
    if (hipStreamCreateWithFlags(&cs, hipStreamNonBlocking) != hipSuccess) return -3;
    hipError_t err = hipMemcpyAsync(stamps, e->prof, words * 8, hipMemcpyDeviceToHost, cs);
    if (err == hipSuccess) err = hipStreamSynchronize(cs);
    (void)hipStreamDestroy(cs);
    host_ns2[0] = e->host_ns[0];
    host_ns2[1] = e->host_ns[1];
    return err == hipSuccess ? e->grid : (int)err;
}
#endif

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
