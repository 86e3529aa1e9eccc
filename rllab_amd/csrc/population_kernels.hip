// population_kernels.hip -- the fused rollout with one parameter vector per env (rl_rollout_population).
//
// The inner loop of the cross-entropy method (rllab/algos/cem.py:29-56: set_param_values(candidate), rollout, return of
// the path) for a whole population in one launch: the per-lane horizon loop of lane_rollout.h (one wavefront per workgroup
// of 64 envs, every lane steps its env through the single-source Env::reset / step / observe, so the host build of the same
// headers replays the launch bit for bit) with the policy below.  Local to this file: lane i evaluates the two-layer MLP of
// ITS candidate c = i % n_cand with plain float32 FMAs, and accumulates the returns of its env's first path.  The
// population arrives transposed, theta_pop_T[P][n_cand], so lanes i, i + 1 read adjacent floats of one row: every weight
// load of the wavefront is one coalesced row segment (two at the wrap of i % n_cand), addressed as scalar row base +
// 32-bit lane offset (RowWalk; it and the first-path sums live in population_lane.h, shared with population_gru_kernels.hip).
//
// Registers: the hidden activations h0 live in LDS as [H][64] floats (lane l only ever touches column l: no bank conflict,
// no synchronisation), the unit loops run at run time over blocks of UB units whose accumulators are named registers --
// no register array is indexed at run time, nothing of the policy is alive while the physics runs.
// Build with -ffp-contract=on like env_kernels.hip (the env arithmetic must match the host oracle build).
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include "../../include/rllab_amd.h"
#include "capi_util.h"
#include "device_rng.h"
#include "envs.h"
#include "lane_rollout.h"
#include "policy_mfma.h"
#include "population_lane.h"

namespace rl {

constexpr int POP_BLOCK = 64;   // one wavefront per workgroup, one env per lane
constexpr int UB = 4;           // hidden units evaluated together (independent FMA chains sharing the input reads)

struct PopulationDev : LaneRolloutDev {
    int n_cand, ident1;
    float log_min_std;
    double discount;
    const float* theta_T;
    float* first_path;
};

// mean = Wout^T act1(W1^T tanh(W0^T o + b0) + b1) + bout of this lane's candidate (network.py:36-101), float32 FMAs in the
// order of the input index.  h0: this lane's column of the [H][64] LDS tile.  ident1: the second layer is the identity
// layer the kernel copy of a one-hidden-layer policy carries (W1 = I, b1 = 0: products with 1 and 0, h1 = h0 exactly).
template <class Env, int H>
__device__ __forceinline__ void population_forward(const float* __restrict__ theta_T, size_t row_bytes, uint32_t& cand_bytes,
                                                   const float* o, float* h0, bool ident1, float* mean) {
    using N = Net<Env::OBS, Env::ACT, H>;
    constexpr int DO = Env::OBS, DA = Env::ACT;
    static_assert(H % UB == 0, "unit blocks");
    {
        RowWalk b0(theta_T, row_bytes, N::B0), w0(theta_T, row_bytes, N::W0);
#pragma unroll 1
        for (int j = 0; j < H; j += UB) {
            float acc[UB];
#pragma unroll
            for (int u = 0; u < UB; ++u) acc[u] = b0.next(row_bytes, cand_bytes);
#pragma unroll
            for (int d = 0; d < DO; ++d) {
#pragma unroll
                for (int u = 0; u < UB; ++u) acc[u] = __builtin_fmaf(o[d], w0.next(row_bytes, cand_bytes), acc[u]);
                w0.skip((size_t)(H - UB) * row_bytes);                    // row W0[d + 1][j]
            }
            w0.skip((size_t)0 - (size_t)(DO * H - UB) * row_bytes);       // row W0[0][j + UB]
#pragma unroll
            for (int u = 0; u < UB; ++u) h0[(j + u) * WV] = ftanh(acc[u]);
        }
    }
    RowWalk b1(theta_T, row_bytes, N::B1), w1(theta_T, row_bytes, N::W1), w2(theta_T, row_bytes, N::W2);
    {
        RowWalk b2(theta_T, row_bytes, N::B2);
#pragma unroll
        for (int k = 0; k < DA; ++k) mean[k] = b2.next(row_bytes, cand_bytes);
    }
#pragma unroll 1
    for (int j = 0; j < H; j += UB) {
        float acc[UB];
#pragma unroll
        for (int u = 0; u < UB; ++u) acc[u] = b1.next(row_bytes, cand_bytes);
#pragma unroll 8
        for (int k = 0; k < H; ++k) {
            const float h = h0[k * WV];
#pragma unroll
            for (int u = 0; u < UB; ++u) acc[u] = __builtin_fmaf(h, w1.next(row_bytes, cand_bytes), acc[u]);
            w1.skip((size_t)(H - UB) * row_bytes);
        }
        w1.skip((size_t)0 - (size_t)(H * H - UB) * row_bytes);
#pragma unroll
        for (int u = 0; u < UB; ++u) {
            const float h1 = ident1 ? acc[u] : ftanh(acc[u]);
#pragma unroll
            for (int k = 0; k < DA; ++k) mean[k] = __builtin_fmaf(h1, w2.next(row_bytes, cand_bytes), mean[k]);   // Wout[j + u][k]
        }
    }
}

// the policy of lane_rollout.h: candidate i % n_cand, always from a reset, and next to it the first path of this env
// (cem.py:46-56: one rollout per candidate, its discounted and undiscounted return)
template <class Env, int H>
struct PopulationPolicy {
    static constexpr bool RECORDS_ALL = false, fresh = true;
    const PopulationDev& a;
    float* const h0;                          // this lane's column of the [H][64] LDS tile
    const size_t row_bytes;
    uint32_t cand_bytes;                      // byte offset of this env's candidate inside a row
    float std_[Env::ACT];
    FirstPath first;

    __device__ __forceinline__ PopulationPolicy(const PopulationDev& a_, int i, float* h0_)
        : a(a_), h0(h0_), row_bytes((size_t)a_.n_cand * sizeof(float)), cand_bytes((uint32_t)(i % a_.n_cand) * 4) {
        // exp(max(log_std, log_min_std)) of this lane's candidate, rounded once from float64 (once per launch)
        RowWalk ls(a.theta_T, row_bytes, Net<Env::OBS, Env::ACT, H>::LSTD);
#pragma unroll
        for (int k = 0; k < Env::ACT; ++k)
            std_[k] = (float)exp((double)fmaxf(ls.next(row_bytes, cand_bytes), a.log_min_std));
    }
    __device__ __forceinline__ float std(int k) const { return std_[k]; }
    __device__ __forceinline__ void restart() {}
    __device__ __forceinline__ void resume(float*) {}
    __device__ __forceinline__ void mean(const float* o, float* m) {
        population_forward<Env, H>(a.theta_T, row_bytes, cand_bytes, o, h0, a.ident1 != 0, m);
    }
    __device__ __forceinline__ void stepped(const float*, float rs, bool d) { first.stepped(rs, d, a.discount); }
    __device__ __forceinline__ void finish(const float*) {}
};

template <class Env, int H>
__global__ void __launch_bounds__(POP_BLOCK) rollout_population_kernel(PopulationDev a) {
    __shared__ float h0_tile[H * WV];
    const int i = blockIdx.x * POP_BLOCK + threadIdx.x;
    if (i >= a.n) return;                     // no cross-lane traffic anywhere: the lanes past the last env just leave
    PopulationPolicy<Env, H> pol(a, i, h0_tile + threadIdx.x);
    rollout_lane<Env>(a, i, pol);
    pol.first.store(a.first_path, a.n, i);
}

template <class Env>
static int launch_population(const rl_population_args* g, hipStream_t st) {
    if (g->hidden != 32 && g->hidden != 64)
        return set_error(RL_ERR_UNSUPPORTED, "rl_rollout_population: hidden = %d (the population kernel is built for 32 and 64)",
                         g->hidden);
    const int act0 = layer_act(RL_ACT_TANH, g->layer_activations, 0), act1 = layer_act(RL_ACT_TANH, g->layer_activations, 1);
    if (act0 != RL_ACT_TANH || (act1 != RL_ACT_TANH && act1 != RL_ACT_IDENTITY) || (g->layer_activations >> 4) != 0)
        return set_error(RL_ERR_UNSUPPORTED, "rl_rollout_population: layer_activations = %d (tanh layers, or tanh + the identity "
                                             "layer of a one-hidden-layer policy)", g->layer_activations);
    PopulationDev a;
    int rc = lane_rollout_dev<Env>(g, (long long)g->n_cand * g->n_evals, "rl_rollout_population", "population kernel", a);
    if (rc) return rc;
    a.n_cand = g->n_cand; a.ident1 = act1 == RL_ACT_IDENTITY ? 1 : 0; a.log_min_std = g->log_min_std;
    a.discount = g->discount; a.theta_T = g->theta_pop_T; a.first_path = g->first_path;
    const dim3 grid((unsigned)((a.n + POP_BLOCK - 1) / POP_BLOCK)), block(POP_BLOCK);
    if (g->hidden == 32) hipLaunchKernelGGL((rollout_population_kernel<Env, 32>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((rollout_population_kernel<Env, 64>), grid, block, 0, st, a);
    return check_launch("rollout_population_kernel");
}

}  // namespace rl

using namespace rl;

extern "C" int rl_rollout_population(const rl_population_args* g, void* stream) {
    if (!g) return set_error(RL_ERR_ARG, "rl_rollout_population: null args");
    if (g->n_cand <= 0 || g->n_evals <= 0 || g->horizon <= 0 || !g->state || !g->ts || !g->theta_pop_T || !g->first_path)
        return set_error(RL_ERR_ARG, "rl_rollout_population: bad argument");
    RL_DISPATCH_ENV(g->kind, launch_population<E>(g, (hipStream_t)stream))
}
