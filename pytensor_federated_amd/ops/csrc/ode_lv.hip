// Native ODE logp+grad for the Lotka-Volterra model family (CDNA4, f64).
//
// Replaces the generic torch forward+discrete-adjoint sweep (models/ode.py:
// ~2500 small kernels per evaluation, 25.6 ms even hipGraph-replayed) with
// TWO kernels: one lane per experiment integrates its whole trajectory
// in-register (RK4, f64), storing states to a scratch slab; the adjoint
// kernel walks the slab backward, recomputing each step's internals and
// applying the hand-derived RK4 vector-Jacobian products.
//
//   du/dt = [ alpha x - beta x y,  delta x y - gamma y ],  theta = (a,b,g,d)
//   logp  = sum_obs sum_comp -(y_obs - u)^2 / (2 sigma^2)   (+ const, host)
//
// The discrete adjoint here is EXACT for the discretized system: identical
// math to models/ode.py's autograd sweep, so the two agree to f64 rounding
// (pinned by tests/test_gpu.py).

#include <hip/hip_runtime.h>

// f(u, theta) and its VJPs
__device__ __forceinline__ void lv_f(double x, double y, const double* th,
                                     double& fx, double& fy) {
    fx = th[0] * x - th[1] * x * y;
    fy = th[3] * x * y - th[2] * y;
}

// (gx, gy) += J_u^T(u) . w ; gth += J_theta^T(u) . w
__device__ __forceinline__ void lv_vjp(double x, double y, const double* th,
                                       double wx, double wy,
                                       double& gx, double& gy, double* gth) {
    gx += (th[0] - th[1] * y) * wx + th[3] * y * wy;
    gy += (-th[1] * x) * wx + (th[3] * x - th[2]) * wy;
    gth[0] += x * wx;
    gth[1] += -x * y * wx;
    gth[2] += -y * wy;
    gth[3] += x * y * wy;
}

// one RK4 step forward from (x,y); returns intermediates for the vjp
struct Rk4Mid {
    double k1x, k1y, k2x, k2y, k3x, k3y, k4x, k4y;
    double u2x, u2y, u3x, u3y, u4x, u4y;
};

__device__ __forceinline__ void rk4_fwd(double x, double y, double h, const double* th,
                                        Rk4Mid& m, double& nx, double& ny) {
    lv_f(x, y, th, m.k1x, m.k1y);
    m.u2x = x + 0.5 * h * m.k1x;
    m.u2y = y + 0.5 * h * m.k1y;
    lv_f(m.u2x, m.u2y, th, m.k2x, m.k2y);
    m.u3x = x + 0.5 * h * m.k2x;
    m.u3y = y + 0.5 * h * m.k2y;
    lv_f(m.u3x, m.u3y, th, m.k3x, m.k3y);
    m.u4x = x + h * m.k3x;
    m.u4y = y + h * m.k3y;
    lv_f(m.u4x, m.u4y, th, m.k4x, m.k4y);
    nx = x + (h / 6.0) * (m.k1x + 2 * m.k2x + 2 * m.k3x + m.k4x);
    ny = y + (h / 6.0) * (m.k1y + 2 * m.k2y + 2 * m.k3y + m.k4y);
}

__device__ __forceinline__ double block_sum_f64(double v, double* lds) {
    const int lane = threadIdx.x & 63;
    const int wid = threadIdx.x >> 6;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if (lane == 0) lds[wid] = v;
    __syncthreads();
    double total = 0.0;
    if (threadIdx.x == 0)
        for (int w = 0; w < (int)(blockDim.x >> 6); ++w) total += lds[w];
    __syncthreads();
    return total;  // valid in thread 0
}

// forward sweep: states + logp
__global__ __launch_bounds__(256) void k_lv_forward(
    const double* __restrict__ u0,       // [B][2]
    const double* __restrict__ y_obs,    // [n_obs][B][2]
    const int* __restrict__ obs_of_step, // [n_steps+1] -> obs index or -1
    int n_steps,
    int B,
    double h,
    double inv_sig2,
    const double* __restrict__ theta,    // [4] device
    double* __restrict__ states,         // [n_steps+1][B][2] scratch
    double* __restrict__ out             // [5] pre-zeroed: logp, g_theta[4]
) {
    double th[4] = {theta[0], theta[1], theta[2], theta[3]};
    double logp_acc = 0.0;
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < B;
         e += gridDim.x * blockDim.x) {
        double x = u0[2 * e], y = u0[2 * e + 1];
        states[2 * e] = x;
        states[2 * e + 1] = y;
        if (obs_of_step[0] >= 0) {
            const double* yo = y_obs + (size_t)obs_of_step[0] * B * 2 + 2 * e;
            const double rx = yo[0] - x, ry = yo[1] - y;
            logp_acc -= 0.5 * inv_sig2 * (rx * rx + ry * ry);
        }
        for (int s = 1; s <= n_steps; ++s) {
            Rk4Mid m;
            double nx, ny;
            rk4_fwd(x, y, h, th, m, nx, ny);
            x = nx;
            y = ny;
            double* st = states + (size_t)s * B * 2 + 2 * e;
            st[0] = x;
            st[1] = y;
            const int j = obs_of_step[s];
            if (j >= 0) {
                const double* yo = y_obs + (size_t)j * B * 2 + 2 * e;
                const double rx = yo[0] - x, ry = yo[1] - y;
                logp_acc -= 0.5 * inv_sig2 * (rx * rx + ry * ry);
            }
        }
    }
    __shared__ double lds[8];
    const double total = block_sum_f64(logp_acc, lds);
    if (threadIdx.x == 0) atomicAdd(&out[0], total);
}

// adjoint sweep: g_theta
__global__ __launch_bounds__(256) void k_lv_adjoint(
    const double* __restrict__ y_obs,
    const int* __restrict__ obs_of_step,
    int n_steps,
    int B,
    double h,
    double inv_sig2,
    const double* __restrict__ theta,
    const double* __restrict__ states,
    double* __restrict__ out  // [5]: logp, g_theta[4]
) {
    double th[4] = {theta[0], theta[1], theta[2], theta[3]};
    double gth[4] = {0, 0, 0, 0};
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < B;
         e += gridDim.x * blockDim.x) {
        double lx = 0.0, ly = 0.0;  // adjoint state dL/du
        {
            const int j = obs_of_step[n_steps];
            if (j >= 0) {
                const double* st = states + (size_t)n_steps * B * 2 + 2 * e;
                const double* yo = y_obs + (size_t)j * B * 2 + 2 * e;
                lx += inv_sig2 * (yo[0] - st[0]);
                ly += inv_sig2 * (yo[1] - st[1]);
            }
        }
        for (int s = n_steps - 1; s >= 0; --s) {
            const double* st = states + (size_t)s * B * 2 + 2 * e;
            const double x = st[0], y = st[1];
            Rk4Mid m;
            double nx, ny;
            rk4_fwd(x, y, h, th, m, nx, ny);  // recompute step internals
            // u_{n+1} = u_n + h/6 (k1 + 2k2 + 2k3 + k4); cotangent = (lx, ly)
            const double w1 = h / 6.0, w24 = h / 3.0;
            double gx = 0, gy = 0;  // accumulates dL/du_n beyond the identity
            // k4 = f(u4), u4 = u_n + h k3
            double g4x = 0, g4y = 0;
            lv_vjp(m.u4x, m.u4y, th, w1 * lx, w1 * ly, g4x, g4y, gth);
            gx += g4x;
            gy += g4y;
            // k3 cotangent: w3 + h * g4
            double c3x = w24 * lx + h * g4x, c3y = w24 * ly + h * g4y;
            double g3x = 0, g3y = 0;
            lv_vjp(m.u3x, m.u3y, th, c3x, c3y, g3x, g3y, gth);
            gx += g3x;
            gy += g3y;
            double c2x = w24 * lx + 0.5 * h * g3x, c2y = w24 * ly + 0.5 * h * g3y;
            double g2x = 0, g2y = 0;
            lv_vjp(m.u2x, m.u2y, th, c2x, c2y, g2x, g2y, gth);
            gx += g2x;
            gy += g2y;
            double c1x = w1 * lx + 0.5 * h * g2x, c1y = w1 * ly + 0.5 * h * g2y;
            double g1x = 0, g1y = 0;
            lv_vjp(x, y, th, c1x, c1y, g1x, g1y, gth);
            gx += g1x;
            gy += g1y;
            lx += gx;
            ly += gy;
            const int j = obs_of_step[s];
            if (j >= 0) {
                const double* yo = y_obs + (size_t)j * B * 2 + 2 * e;
                lx += inv_sig2 * (yo[0] - x);
                ly += inv_sig2 * (yo[1] - y);
            }
        }
    }
    __shared__ double lds[8];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double total = block_sum_f64(gth[k], lds);
        if (threadIdx.x == 0) atomicAdd(&out[1 + k], total);
        __syncthreads();
    }
}

// Batched variant: C chains (thetas) x B experiments in one sweep.  Lane
// l handles (chain = l / B, experiment = l % B) for any B and C: there is no
// block reduction here, every lane adds its own contribution to its chain's
// output slot atomically, so a block may hold lanes of several chains.
// Fills the chip (B*C lanes) where the single-theta kernel at B=1024 only
// occupies 4 CUs.
__global__ __launch_bounds__(256) void k_lv_forward_batched(
    const double* __restrict__ u0,       // [B][2]
    const double* __restrict__ y_obs,    // [n_obs][B][2]
    const int* __restrict__ obs_of_step,
    int n_steps, int B, int n_chains,
    double h, double inv_sig2,
    const double* __restrict__ theta,    // [C][4]
    double* __restrict__ states,         // [C][n_steps+1][B][2]
    double* __restrict__ out             // [C][5] pre-zeroed
) {
    const long long total = (long long)B * n_chains;
    for (long long l = blockIdx.x * blockDim.x + threadIdx.x; l < total;
         l += (long long)gridDim.x * blockDim.x) {
        const int ch = (int)(l / B);
        const int e = (int)(l % B);
        const double* th = theta + 4 * ch;
        double thr[4] = {th[0], th[1], th[2], th[3]};
        double* st_base = states + (size_t)ch * (n_steps + 1) * B * 2;
        double x = u0[2 * e], y = u0[2 * e + 1];
        st_base[2 * e] = x;
        st_base[2 * e + 1] = y;
        double logp_acc = 0.0;
        if (obs_of_step[0] >= 0) {
            const double* yo = y_obs + (size_t)obs_of_step[0] * B * 2 + 2 * e;
            const double rx = yo[0] - x, ry = yo[1] - y;
            logp_acc -= 0.5 * inv_sig2 * (rx * rx + ry * ry);
        }
        for (int s = 1; s <= n_steps; ++s) {
            Rk4Mid m;
            double nx, ny;
            rk4_fwd(x, y, h, thr, m, nx, ny);
            x = nx;
            y = ny;
            double* st = st_base + (size_t)s * B * 2 + 2 * e;
            st[0] = x;
            st[1] = y;
            const int j = obs_of_step[s];
            if (j >= 0) {
                const double* yo = y_obs + (size_t)j * B * 2 + 2 * e;
                const double rx = yo[0] - x, ry = yo[1] - y;
                logp_acc -= 0.5 * inv_sig2 * (rx * rx + ry * ry);
            }
        }
        // per-lane atomic into the chain slot (few k lanes per chain; the
        // f64 atomic rate is ample at this arithmetic intensity)
        atomicAdd(&out[5 * ch], logp_acc);
    }
}

__global__ __launch_bounds__(256) void k_lv_adjoint_batched(
    const double* __restrict__ y_obs,
    const int* __restrict__ obs_of_step,
    int n_steps, int B, int n_chains,
    double h, double inv_sig2,
    const double* __restrict__ theta,
    const double* __restrict__ states,
    double* __restrict__ out  // [C][5]
) {
    const long long total = (long long)B * n_chains;
    for (long long l = blockIdx.x * blockDim.x + threadIdx.x; l < total;
         l += (long long)gridDim.x * blockDim.x) {
        const int ch = (int)(l / B);
        const int e = (int)(l % B);
        const double* th = theta + 4 * ch;
        double thr[4] = {th[0], th[1], th[2], th[3]};
        const double* st_base = states + (size_t)ch * (n_steps + 1) * B * 2;
        double gth[4] = {0, 0, 0, 0};
        double lx = 0.0, ly = 0.0;
        {
            const int j = obs_of_step[n_steps];
            if (j >= 0) {
                const double* st = st_base + (size_t)n_steps * B * 2 + 2 * e;
                const double* yo = y_obs + (size_t)j * B * 2 + 2 * e;
                lx += inv_sig2 * (yo[0] - st[0]);
                ly += inv_sig2 * (yo[1] - st[1]);
            }
        }
        for (int s = n_steps - 1; s >= 0; --s) {
            const double* st = st_base + (size_t)s * B * 2 + 2 * e;
            const double x = st[0], y = st[1];
            Rk4Mid m;
            double nx, ny;
            rk4_fwd(x, y, h, thr, m, nx, ny);
            const double w1 = h / 6.0, w24 = h / 3.0;
            double gx = 0, gy = 0;
            double g4x = 0, g4y = 0;
            lv_vjp(m.u4x, m.u4y, thr, w1 * lx, w1 * ly, g4x, g4y, gth);
            gx += g4x;
            gy += g4y;
            double c3x = w24 * lx + h * g4x, c3y = w24 * ly + h * g4y;
            double g3x = 0, g3y = 0;
            lv_vjp(m.u3x, m.u3y, thr, c3x, c3y, g3x, g3y, gth);
            gx += g3x;
            gy += g3y;
            double c2x = w24 * lx + 0.5 * h * g3x, c2y = w24 * ly + 0.5 * h * g3y;
            double g2x = 0, g2y = 0;
            lv_vjp(m.u2x, m.u2y, thr, c2x, c2y, g2x, g2y, gth);
            gx += g2x;
            gy += g2y;
            double c1x = w1 * lx + 0.5 * h * g2x, c1y = w1 * ly + 0.5 * h * g2y;
            double g1x = 0, g1y = 0;
            lv_vjp(x, y, thr, c1x, c1y, g1x, g1y, gth);
            gx += g1x;
            gy += g1y;
            lx += gx;
            ly += gy;
            const int j = obs_of_step[s];
            if (j >= 0) {
                const double* yo = y_obs + (size_t)j * B * 2 + 2 * e;
                lx += inv_sig2 * (yo[0] - x);
                ly += inv_sig2 * (yo[1] - y);
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) atomicAdd(&out[5 * ch + 1 + k], gth[k]);
    }
}

extern "C" int fed_ode_lv_eval_batched(
    const double* u0, const double* y_obs, const int* obs_of_step,
    int n_steps, int B, int n_chains, double h, double sigma,
    const double* theta_dev,  // [C][4]
    double* states_ws, double* out, void* stream_v
) {
    hipStream_t stream = (hipStream_t)stream_v;
    hipError_t err = hipMemsetAsync(out, 0, (size_t)n_chains * 5 * sizeof(double), stream);
    if (err != hipSuccess) return (int)err;
    const double inv_sig2 = 1.0 / (sigma * sigma);
    long long total = (long long)B * n_chains;
    int grid = (int)((total + 255) / 256);
    if (grid > 2048) grid = 2048;
    hipLaunchKernelGGL(k_lv_forward_batched, dim3(grid), dim3(256), 0, stream,
                       u0, y_obs, obs_of_step, n_steps, B, n_chains, h, inv_sig2,
                       theta_dev, states_ws, out);
    hipError_t e1 = hipGetLastError();
    if (e1 != hipSuccess) return (int)e1;
    hipLaunchKernelGGL(k_lv_adjoint_batched, dim3(grid), dim3(256), 0, stream,
                       y_obs, obs_of_step, n_steps, B, n_chains, h, inv_sig2,
                       theta_dev, states_ws, out);
    return (int)hipGetLastError();
}

extern "C" int fed_ode_lv_eval(
    const double* u0, const double* y_obs, const int* obs_of_step,
    int n_steps, int B, double h, double sigma,
    const double* theta_dev,
    double* states_ws, double* out5, void* stream_v
) {
    hipStream_t stream = (hipStream_t)stream_v;
    hipError_t err = hipMemsetAsync(out5, 0, 5 * sizeof(double), stream);
    if (err != hipSuccess) return (int)err;
    const double inv_sig2 = 1.0 / (sigma * sigma);
    int grid = (B + 255) / 256;
    if (grid > 1024) grid = 1024;
    hipLaunchKernelGGL(k_lv_forward, dim3(grid), dim3(256), 0, stream,
                       u0, y_obs, obs_of_step, n_steps, B, h, inv_sig2,
                       theta_dev, states_ws, out5);
    hipError_t e1 = hipGetLastError();
    if (e1 != hipSuccess) return (int)e1;
    hipLaunchKernelGGL(k_lv_adjoint, dim3(grid), dim3(256), 0, stream,
                       y_obs, obs_of_step, n_steps, B, h, inv_sig2,
                       theta_dev, states_ws, out5);
    return (int)hipGetLastError();
}
