// Host-side glue of the row-group entry points fed_glm_family (glm_family.hip)
// and fed_glm_family_fvp (glm_family_fvp.hip): the launch plan and the
// (dtype, link, K) -> kernel instantiation switch.  The kernels' common block
// epilogue is not here: a shared device helper changed their ISA (note in
// k_glm_family).

#pragma once

#include <type_traits>

#include "fed_common.hpp"
#include "glm_links.hpp"

struct RowGroupPlan {
    int grid, block, rows_per_step;
};

// Argument checks, grid choice and workspace shrink.  Returns 0, or in the
// order checked: -2 bad dtype, -5 unknown link, -4 unsupported K, -3
// workspace too small.  Writes and launches nothing.
static inline int plan_row_group(int dtype, int link, int K, long long n_rows, long long ws_bytes,
                                 RowGroupPlan& plan) {
    if (dtype != FED_BF16 && dtype != FED_F32) return -2;
    if (link != FED_LINK_POISSON && link != FED_LINK_GAUSSIAN && link != FED_LINK_LOGISTIC)
        return -5;
    const int vec = dtype == FED_BF16 ? 8 : 4;
    if (K < vec || K % vec != 0) return -4;
    const int lanes = K / vec;  // G, or 64*KITER
    if (lanes > 256 || (lanes & (lanes - 1)) != 0) return -4;
    plan.rows_per_step = lanes >= WAVE ? 1 : WAVE / lanes;
    plan.block = 256;
    const int waves_per_block = plan.block / WAVE;
    const long long steps = (n_rows + plan.rows_per_step - 1) / plan.rows_per_step;
    const long long pairs = (steps + 1) / 2;
    int grid = pick_grid(pairs / waves_per_block + 1, 1);
    if (grid > 1024) grid = 1024;
    // FED_GLM_GRID caps the grid (tests reach a second grid-stride trip at
    // small N with it); read per call
    if (const char* ge = getenv("FED_GLM_GRID")) {
        const int v = atoi(ge);
        if (v >= 1 && v < grid) grid = v;
    }
    const long long need = (long long)grid * K * sizeof(float);
    if (need > ws_bytes) grid = (int)(ws_bytes / ((long long)K * sizeof(float)));
    if (grid < 1) return -3;
    plan.grid = grid;
    return 0;
}

template <int N>
using int_c = std::integral_constant<int, N>;
template <class T>
struct type_c { using type = T; };

// (dtype, link, K) -> (T, Link, G, KITER), K / VEC = G * KITER: calls
// f(type_c<T>, type_c<Link>, int_c<G>, int_c<KITER>) and returns 0, or -4
// when K is not compiled.  dtype, link and K % VEC == 0 are plan_row_group's
// checks.
template <class F>
static int dispatch_row_group(int dtype, int link, int K, F&& f) {
    const auto with_k = [&](auto t, auto l) {
        const auto go = [&](auto g, auto kiter) { f(t, l, g, kiter); return 0; };
        switch (K / VecTraits<typename decltype(t)::type>::VEC) {
            case 1:   return go(int_c<1>{}, int_c<1>{});
            case 2:   return go(int_c<2>{}, int_c<1>{});
            case 4:   return go(int_c<4>{}, int_c<1>{});
            case 8:   return go(int_c<8>{}, int_c<1>{});
            case 16:  return go(int_c<16>{}, int_c<1>{});
            case 32:  return go(int_c<32>{}, int_c<1>{});
            case 64:  return go(int_c<64>{}, int_c<1>{});
            case 128: return go(int_c<64>{}, int_c<2>{});
            case 256: return go(int_c<64>{}, int_c<4>{});
            default:  return -4;
        }
    };
    const auto with_dtype = [&](auto l) {
        return dtype == FED_BF16 ? with_k(type_c<bf16_tag>{}, l) : with_k(type_c<float>{}, l);
    };
    switch (link) {
        case FED_LINK_POISSON:  return with_dtype(type_c<PoissonLink>{});
        case FED_LINK_GAUSSIAN: return with_dtype(type_c<GaussianLink>{});
        default:                return with_dtype(type_c<LogisticLink>{});
    }
}
