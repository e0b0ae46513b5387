// Link policies of the GLM family kernels: what turns the linear predictor
// z = x.beta (+ offset) of one row into its logp term and its residual
// d term / d z (eval), and into its Fisher weight -d^2 term / dz^2 (weight;
// used by glm_family_fisher.hip, Poisson and Gaussian, and by
// glm_family_fvp.hip, all three).  Shared by the single-chain kernel (glm_family.hip) and the
// 16-chain MFMA kernel (glm_family_batched.hip), so both evaluate a row by
// the same expressions in the same order.
//   Poisson  (log link)   term = y*z - exp(z)         resid = y - exp(z)
//   Gaussian (identity)   term = -r*r/(2 sigma^2)     resid = r/sigma^2, r = y-z
//   Logistic              the expressions of k_logistic_glm_reg, in its order

#pragma once

#include <hip/hip_runtime.h>

enum FedLink { FED_LINK_POISSON = 0, FED_LINK_GAUSSIAN = 1, FED_LINK_LOGISTIC = 2 };

struct LinkParams {
    float inv_s2;       // 1 / sigma^2       (Gaussian)
    float half_inv_s2;  // 1 / (2 sigma^2)   (Gaussian)
};

static inline LinkParams make_link_params(double sigma) {
    LinkParams lp;
    lp.inv_s2 = (float)(1.0 / (sigma * sigma));
    lp.half_inv_s2 = (float)(0.5 / (sigma * sigma));
    return lp;
}

struct PoissonLink {
    __device__ static __forceinline__ void eval(float y, float z, const LinkParams&,
                                                float& term, float& resid) {
        const float mu = __expf(z);  // z > 88: mu = inf, term = -inf (documented)
        term = y * z - mu;
        resid = y - mu;
    }
    // w = -d^2 term / dz^2 (the Fisher kernel's row weight)
    __device__ static __forceinline__ void weight(float z, const LinkParams&, float& w) {
        w = __expf(z);
    }
};

struct GaussianLink {
    __device__ static __forceinline__ void eval(float y, float z, const LinkParams& p,
                                                float& term, float& resid) {
        const float r = y - z;
        term = -(r * r) * p.half_inv_s2;
        resid = r * p.inv_s2;
    }
    __device__ static __forceinline__ void weight(float, const LinkParams& p, float& w) {
        w = p.inv_s2;
    }
};

struct LogisticLink {
    __device__ static __forceinline__ void eval(float y, float z, const LinkParams&,
                                                float& term, float& resid) {
        // stable: y*z - softplus(z) = y*z - (max(z,0) + log1p(exp(-|z|)))
        const float sp = fmaxf(z, 0.f) + log1pf(__expf(-fabsf(z)));
        term = y * z - sp;
        resid = y - 1.f / (1.f + __expf(-z));
    }
    // w = mu * (1 - mu), mu formed as eval forms it (glm_family_fvp.hip; the
    // Fisher MFMA kernel has no logistic weight)
    __device__ static __forceinline__ void weight(float z, const LinkParams&, float& w) {
        const float mu = 1.f / (1.f + __expf(-z));
        w = mu * (1.f - mu);
    }
};
