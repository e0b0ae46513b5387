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

// Middle stages of k_glm_family_batched: what a thread does with the z of
// its (row, column) slot.  A stage names its Params (a kernel argument) and
// gives eval(y, z, column, params, term, resid).
//
// ElementStage<Link>: the 16 columns are 16 independent chains and a slot is
// evaluated on its own, by Link::eval.
template <class Link>
struct ElementStage {
    using Params = LinkParams;
    __device__ static __forceinline__ void eval(float y, float z, int, const Params& p,
                                                float& term, float& resid) {
        Link::eval(y, z, p, term, resid);
    }
};

// SoftmaxStage (multinomial logit): the 16 columns are 16/cp chains of cp
// class slots each, cp the next power of two >= n_classes; column g*cp + c
// is class c of chain g and y is the row's label.  The slots of a row are
// coupled by a log-sum-exp over their class group:
//     m = max_c z_c   e_c = exp(z_c - m)   s = sum_c e_c   p_c = e_c / s
//     resid_c = [c == y] - p_c       term = (z_y - m) - log(s) on the lane c == y
// A padded class (c >= n_classes) takes z = -inf: e = 0, resid = 0.  The
// group sits in cp adjacent lanes (column = lane & 15), so both reductions
// are butterflies of log2(cp) steps inside a 16-lane DPP row; every lane of
// the wave must call eval together.  Subtracting m keeps |z| in the
// thousands finite.
//
// The butterfly is DPP (data-parallel primitives on the operand read, no
// LDS crossbar): lane ^ 1 and lane ^ 2 by quad_perm, then row_half_mirror
// (lane -> 7 - lane of its 8) and row_mirror (lane -> 15 - lane of its 16).
// A mirror is no xor, but after the earlier steps all lanes of a quad (of
// an 8) hold one value, so it delivers the other half's value all the same;
// both operands of a step are the same two numbers on both sides, so the
// lanes of a group end with bit-identical m and s.  The steps at or past cp
// are masked.  It replaced a __shfl_xor butterfly (ds_bpermute_b32) after
// an alternating A/B: profiles/PROFILES.md "Softmax GLM".
struct SoftmaxParams {
    int n_classes;  // C in [2, 16]
    int cp;         // class-group width: 2, 4, 8 or 16 (wave-uniform)
};

// dpp_ctrl encodings of the CDNA ISA
enum : int {
    DPP_XOR1 = 0xB1,         // quad_perm:[1,0,3,2]
    DPP_XOR2 = 0x4E,         // quad_perm:[2,3,0,1]
    DPP_HALF_MIRROR = 0x141, // row_half_mirror
    DPP_MIRROR = 0x140,      // row_mirror
};

template <int CTRL>
__device__ __forceinline__ float dpp_f32(float v) {
    return __int_as_float(
        __builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false));
}

struct SoftmaxStage {
    using Params = SoftmaxParams;
    __device__ static __forceinline__ void eval(float y, float z, int column, const Params& p,
                                                float& term, float& resid) {
        const int c = column & (p.cp - 1);
        if (c >= p.n_classes) z = -INFINITY;
        float m = z;
        m = fmaxf(m, dpp_f32<DPP_XOR1>(m));
        { const float o = dpp_f32<DPP_XOR2>(m); if (2 < p.cp) m = fmaxf(m, o); }
        { const float o = dpp_f32<DPP_HALF_MIRROR>(m); if (4 < p.cp) m = fmaxf(m, o); }
        { const float o = dpp_f32<DPP_MIRROR>(m); if (8 < p.cp) m = fmaxf(m, o); }
        const float e = __expf(z - m);
        float s = e;
        s += dpp_f32<DPP_XOR1>(s);
        { const float o = dpp_f32<DPP_XOR2>(s); if (2 < p.cp) s += o; }
        { const float o = dpp_f32<DPP_HALF_MIRROR>(s); if (4 < p.cp) s += o; }
        { const float o = dpp_f32<DPP_MIRROR>(s); if (8 < p.cp) s += o; }
        const bool hit = (float)c == y;
        resid = (hit ? 1.f : 0.f) - e / s;
        term = hit ? (z - m) - __logf(s) : 0.f;
    }
};
