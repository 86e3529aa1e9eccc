// categorical_kernels.hip -- discrete actions: the fused GridWorld rollout and the categorical head of the policy
// objectives on PLANES (CategoricalMLPPolicy on GridWorldEnv, rllab/policies/categorical_mlp_policy.py:15-85,
// rllab/envs/grid_world_env.py:36-149, rllab/distributions/categorical.py:23-87).
//
//   rl_rollout_gridworld   : one lane per env, the whole horizon in one launch.  Observations are one-hot, so the
//                            policy is a function of the state index alone: the launch reads a probability table
//                            prob[n_act][n_states] the caller builds once per parameter version.  Per step: record the
//                            one-hot observation, draw one uniform (the env's Philox stream, or an injected plane),
//                            k = #{j : cs_j < u} clamped to n_act - 1 with cs the float32 running sum of the state's
//                            row in index order (rllab/misc/special.py:10-19), the transition of
//                            get_possible_next_states / step, then the VecEnvExecutor contract (ts += 1,
//                            done |= ts >= max_path_length, a done env restarts at start_state with ts = 0).
//   rl_categorical_softmax : prob = softmax(logits) on planes [n_act][B], max-subtracted (the table above).
//   rl_categorical_head    : from logits planes of the current parameters and the recorded batch,
//                              out4 = [ sum w lr adv, sum w KL(old || new), sum w logp adv, max KL ]
//                            lr = (p_new.a + TINY) / (p_old.a + TINY), KL = sum_k p_old (log(p_old + TINY) - log(p_new + TINY)),
//                            logp = log(p_new.a + TINY), and the cotangent on the logits of
//                              (-sum w {lr | logp} adv + kl_penalty sum w KL) * inv_count,   softmax Jacobian included.
//   rl_categorical_fisher  : g = w inv_count H dlogits, H the Hessian of the per-sample KL above in the new logits at
//                            new == old, TINY kept:  with G_k = -p_k / (p_k + TINY), D_k = p_k / (p_k + TINY)^2,
//                            dp = J dlogits, J = diag(p) - p p^T:
//                              H dlogits = J^T (D dp)  +  G dp - p (G.dp) - (G.p) dp
//                            (the second group vanishes at TINY = 0, where H = diag(p) - p p^T).
// The head arithmetic is float64 on float32 planes: HBM-bound (~ (3 A + 2) floats in, A floats out per sample), and
// the sums then carry the rounding of the logits alone.
#include <hip/hip_runtime.h>
#include "../../include/rllab_amd.h"
#include "capi_util.h"
#include "device_rng.h"
#include "gridworld_lane.h"

namespace rl {

int launch_reduce_loss(const double* partial, int rows, double* out, hipStream_t st);   // policy_kernels.hip

constexpr int CAT_THREADS = 256;
constexpr int CAT_MAX_ACT = 8;
constexpr int CAT_MAX_GRID = 1024;
constexpr double CAT_TINY = 1e-8;
constexpr int GRID_MAX_STATES = 1024;
constexpr int GRID_THREADS = 64;

// ---------------------------------------------------------------------------------------------------------------------
// GridWorld rollout
// ---------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(GRID_THREADS) gridworld_rollout_kernel(rl_gridworld_args a) {
    const int i = blockIdx.x * GRID_THREADS + threadIdx.x;
    const int n = a.n_envs;
    if (i >= n) return;
    const int S = a.n_row * a.n_col, T = a.horizon;
    int s = a.reset_at_start ? a.start_state : a.state[i];
    int ts = a.reset_at_start ? 0 : a.ts[i];
    s = s < 0 ? 0 : (s >= S ? S - 1 : s);              // (a caller's state array is not trusted with an index)
    for (int t = 0; t < T; ++t) {
        const size_t col = (size_t)t * n + i;
        for (int k = 0; k < S; ++k) a.obs[((size_t)k * T + t) * n + i] = (k == s) ? 1.0f : 0.0f;
        float p[GRID_ACTIONS];
#pragma unroll
        for (int k = 0; k < GRID_ACTIONS; ++k) p[k] = a.prob[(size_t)k * S + s];
        float u;
        if (a.u) u = a.u[col];
        else philox_draws<1, false>(&u, a.seed, (uint32_t)(a.env_offset + i), a.step_counter + (uint64_t)t, RNG_POLICY);
        const int act = grid_weighted_sample(p, u);
#pragma unroll
        for (int k = 0; k < GRID_ACTIONS; ++k) {
            a.actions[((size_t)k * T + t) * n + i] = (k == act) ? 1.0f : 0.0f;
            a.prob_out[((size_t)k * T + t) * n + i] = p[k];
        }
        bool done;
        float reward;
        const int ns = grid_transition(a.cell, a.n_row, a.n_col, s, act, done, reward);
        ts += 1;
        if (a.max_path_length > 0 && ts >= a.max_path_length) done = true;
        a.rewards[col] = reward;
        a.dones[col] = done ? 1 : 0;
        if (done) {
            s = a.start_state;
            ts = 0;
        } else {
            s = ns;
        }
    }
    a.state[i] = s;
    a.ts[i] = ts;
}

// ---------------------------------------------------------------------------------------------------------------------
// categorical head
// ---------------------------------------------------------------------------------------------------------------------
// p[0..A) = softmax of the sample's logits column, max-subtracted, float64
__device__ __forceinline__ void softmax_column(const float* __restrict__ logits, size_t B, size_t b, int A, double* p) {
    double m = -INFINITY;
#pragma unroll
    for (int k = 0; k < CAT_MAX_ACT; ++k)
        if (k < A) {
            p[k] = (double)logits[(size_t)k * B + b];
            m = fmax(m, p[k]);
        }
    double z = 0.0;
#pragma unroll
    for (int k = 0; k < CAT_MAX_ACT; ++k)
        if (k < A) {
            p[k] = exp(p[k] - m);
            z += p[k];
        }
    const double iz = 1.0 / z;
#pragma unroll
    for (int k = 0; k < CAT_MAX_ACT; ++k)
        if (k < A) p[k] *= iz;
}

__global__ void __launch_bounds__(CAT_THREADS) categorical_softmax_kernel(size_t B, int A, const float* __restrict__ logits,
                                                                          float* __restrict__ prob) {
    for (size_t b = (size_t)blockIdx.x * CAT_THREADS + threadIdx.x; b < B; b += (size_t)gridDim.x * CAT_THREADS) {
        double p[CAT_MAX_ACT];
        softmax_column(logits, B, b, A, p);
#pragma unroll
        for (int k = 0; k < CAT_MAX_ACT; ++k)
            if (k < A) prob[(size_t)k * B + b] = (float)p[k];
    }
}

struct CatHeadArgs {
    size_t B;
    int A, vpg;
    const float* logits;      // [A][B] planes
    const float* act;         // one-hot
    const float* adv;
    const float* old_prob;
    const float* w;
    float inv_count, kl_penalty;
    float* g_logits;          // null = sums only
    double* partial;          // [grid][4]
};

__device__ __forceinline__ double cat_block_sum(double v, double* scratch) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
    __syncthreads();
    return (scratch[0] + scratch[1]) + (scratch[2] + scratch[3]);
}

__global__ void __launch_bounds__(CAT_THREADS) categorical_head_kernel(CatHeadArgs a) {
    __shared__ double scratch[4];
    __shared__ double smax[4];
    double s_loss = 0.0, s_kl = 0.0, s_vpg = 0.0, max_kl = -INFINITY;
    const size_t B = a.B;
    const int A = a.A;
    for (size_t b = (size_t)blockIdx.x * CAT_THREADS + threadIdx.x; b < B; b += (size_t)gridDim.x * CAT_THREADS) {
        const double wgt = (double)a.w[b], advb = (double)a.adv[b];
        double p[CAT_MAX_ACT], po[CAT_MAX_ACT], ak[CAT_MAX_ACT];
        softmax_column(a.logits, B, b, A, p);
        double pa = 0.0, poa = 0.0, kl = 0.0;
#pragma unroll
        for (int k = 0; k < CAT_MAX_ACT; ++k)
            if (k < A) {
                const size_t i = (size_t)k * B + b;
                po[k] = (double)a.old_prob[i];
                ak[k] = (double)a.act[i];
                pa += p[k] * ak[k];
                poa += po[k] * ak[k];
                kl += po[k] * (log(po[k] + CAT_TINY) - log(p[k] + CAT_TINY));
            }
        const double lr = (pa + CAT_TINY) / (poa + CAT_TINY);
        const double logp = log(pa + CAT_TINY);
        s_loss += wgt * lr * advb;
        s_kl += wgt * kl;
        s_vpg += wgt * logp * advb;
        if (wgt > 0.0) max_kl = fmax(max_kl, kl);
        if (a.g_logits) {
            // G_k = d objective_b / d p_k, then through the softmax: g_j = p_j (G_j - sum_k p_k G_k)
            const double c = -wgt * advb * (double)a.inv_count / (a.vpg ? (pa + CAT_TINY) : (poa + CAT_TINY));
            const double pen = (double)a.kl_penalty * wgt * (double)a.inv_count;
            double G[CAT_MAX_ACT], pg = 0.0;
#pragma unroll
            for (int k = 0; k < CAT_MAX_ACT; ++k)
                if (k < A) {
                    G[k] = c * ak[k] - pen * po[k] / (p[k] + CAT_TINY);
                    pg += p[k] * G[k];
                }
#pragma unroll
            for (int k = 0; k < CAT_MAX_ACT; ++k)
                if (k < A) a.g_logits[(size_t)k * B + b] = (float)(p[k] * (G[k] - pg));
        }
    }
    const double l = cat_block_sum(s_loss, scratch), k = cat_block_sum(s_kl, scratch), v = cat_block_sum(s_vpg, scratch);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) max_kl = fmax(max_kl, __shfl_xor(max_kl, o, 64));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) smax[threadIdx.x >> 6] = max_kl;
    __syncthreads();
    if (threadIdx.x == 0) {
        double* o = a.partial + (size_t)blockIdx.x * 4;
        o[0] = l; o[1] = k; o[2] = v;
        o[3] = fmax(fmax(smax[0], smax[1]), fmax(smax[2], smax[3]));
    }
}

__global__ void __launch_bounds__(CAT_THREADS) categorical_fisher_kernel(size_t B, int A, const float* __restrict__ dlogits,
                                                                         const float* __restrict__ logits,
                                                                         const float* __restrict__ w, float inv_count,
                                                                         float* __restrict__ g_logits) {
    for (size_t b = (size_t)blockIdx.x * CAT_THREADS + threadIdx.x; b < B; b += (size_t)gridDim.x * CAT_THREADS) {
        const double c = (double)w[b] * (double)inv_count;
        double p[CAT_MAX_ACT], dp[CAT_MAX_ACT], q[CAT_MAX_ACT], G[CAT_MAX_ACT];
        softmax_column(logits, B, b, A, p);
        double pv = 0.0;
#pragma unroll
        for (int k = 0; k < CAT_MAX_ACT; ++k)
            if (k < A) {
                dp[k] = (double)dlogits[(size_t)k * B + b];
                pv += p[k] * dp[k];
            }
        double pq = 0.0, gdp = 0.0, gp = 0.0;
#pragma unroll
        for (int k = 0; k < CAT_MAX_ACT; ++k)
            if (k < A) {
                dp[k] = p[k] * (dp[k] - pv);                   // J dlogits
                const double den = p[k] + CAT_TINY;
                G[k] = -p[k] / den;
                q[k] = p[k] / (den * den) * dp[k];             // D dp
                pq += p[k] * q[k];
                gdp += G[k] * dp[k];
                gp += G[k] * p[k];
            }
#pragma unroll
        for (int k = 0; k < CAT_MAX_ACT; ++k)
            if (k < A)
                g_logits[(size_t)k * B + b] = (float)(c * (p[k] * (q[k] - pq) + G[k] * dp[k] - p[k] * gdp - gp * dp[k]));
    }
}

static int cat_grid(size_t n_samples) {
    const size_t blocks = (n_samples + CAT_THREADS - 1) / CAT_THREADS;
    return (int)(blocks < (size_t)CAT_MAX_GRID ? blocks : (size_t)CAT_MAX_GRID);
}

}  // namespace rl

using namespace rl;

extern "C" int rl_rollout_gridworld(const rl_gridworld_args* args, void* stream) {
    if (!args) return set_error(RL_ERR_ARG, "rl_rollout_gridworld: null arguments");
    const rl_gridworld_args& a = *args;
    if (a.n_envs < 1 || a.horizon < 1) return set_error(RL_ERR_ARG, "rl_rollout_gridworld: zero-sized launch (n_envs %d, horizon %d)", a.n_envs, a.horizon);
    if (a.n_act != GRID_ACTIONS) return set_error(RL_ERR_ARG, "rl_rollout_gridworld: n_act %d (GridWorld has %d actions)", a.n_act, GRID_ACTIONS);
    if (a.n_row < 1 || a.n_col < 1 || (long long)a.n_row * a.n_col > GRID_MAX_STATES)
        return set_error(RL_ERR_ARG, "rl_rollout_gridworld: map %d x %d (1 .. %d states)", a.n_row, a.n_col, GRID_MAX_STATES);
    if (a.start_state < 0 || a.start_state >= a.n_row * a.n_col)
        return set_error(RL_ERR_ARG, "rl_rollout_gridworld: start_state %d outside the map", a.start_state);
    if (a.max_path_length < 0 || a.env_offset < 0) return set_error(RL_ERR_ARG, "rl_rollout_gridworld: negative max_path_length / env_offset");
    if (!a.cell || !a.prob || !a.state || !a.ts || !a.obs || !a.actions || !a.prob_out || !a.rewards || !a.dones)
        return set_error(RL_ERR_ARG, "rl_rollout_gridworld: null pointer");
    const int grid = (a.n_envs + GRID_THREADS - 1) / GRID_THREADS;
    hipLaunchKernelGGL(gridworld_rollout_kernel, dim3(grid), dim3(GRID_THREADS), 0, (hipStream_t)stream, a);
    return check_launch("gridworld_rollout_kernel");
}

extern "C" int rl_categorical_softmax(size_t n_samples, int n_act, const float* logits, float* prob, void* stream) {
    if (n_samples == 0 || n_act < 1 || n_act > CAT_MAX_ACT || !logits || !prob)
        return set_error(RL_ERR_ARG, "rl_categorical_softmax: bad argument (n_samples %zu, n_act %d of 1 .. %d, or a null pointer)",
                         n_samples, n_act, CAT_MAX_ACT);
    hipLaunchKernelGGL(categorical_softmax_kernel, dim3(cat_grid(n_samples)), dim3(CAT_THREADS), 0, (hipStream_t)stream,
                       n_samples, n_act, logits, prob);
    return check_launch("categorical_softmax_kernel");
}

extern "C" size_t rl_categorical_head_workspace_bytes(void) { return (size_t)CAT_MAX_GRID * 4 * sizeof(double); }

extern "C" int rl_categorical_head(size_t n_samples, int n_act, const float* logits, const float* actions,
                                   const float* advantages, const float* old_prob, const float* weights, float inv_count,
                                   int vpg, float kl_penalty, float* g_logits, void* workspace, size_t workspace_bytes,
                                   double* out4, void* stream) {
    if (n_samples == 0 || n_act < 1 || n_act > CAT_MAX_ACT || !logits || !actions || !advantages || !old_prob || !weights ||
        !out4 || !workspace)
        return set_error(RL_ERR_ARG, "rl_categorical_head: bad argument (n_samples %zu, n_act %d of 1 .. %d, or a null pointer)",
                         n_samples, n_act, CAT_MAX_ACT);
    if (workspace_bytes < rl_categorical_head_workspace_bytes())
        return set_error(RL_ERR_ARG, "rl_categorical_head: workspace too small");
    CatHeadArgs a;
    a.B = n_samples; a.A = n_act; a.vpg = vpg; a.logits = logits; a.act = actions; a.adv = advantages;
    a.old_prob = old_prob; a.w = weights; a.inv_count = inv_count; a.kl_penalty = kl_penalty; a.g_logits = g_logits;
    a.partial = (double*)workspace;
    const int grid = cat_grid(n_samples);
    hipLaunchKernelGGL(categorical_head_kernel, dim3(grid), dim3(CAT_THREADS), 0, (hipStream_t)stream, a);
    int rc = check_launch("categorical_head_kernel");
    if (rc) return rc;
    return launch_reduce_loss(a.partial, grid, out4, (hipStream_t)stream);
}

extern "C" int rl_categorical_fisher(size_t n_samples, int n_act, const float* dlogits, const float* logits,
                                     const float* weights, float inv_count, float* g_logits, void* stream) {
    if (n_samples == 0 || n_act < 1 || n_act > CAT_MAX_ACT || !dlogits || !logits || !weights || !g_logits)
        return set_error(RL_ERR_ARG, "rl_categorical_fisher: bad argument (n_samples %zu, n_act %d of 1 .. %d, or a null pointer)",
                         n_samples, n_act, CAT_MAX_ACT);
    hipLaunchKernelGGL(categorical_fisher_kernel, dim3(cat_grid(n_samples)), dim3(CAT_THREADS), 0, (hipStream_t)stream,
                       n_samples, n_act, dlogits, logits, weights, inv_count, g_logits);
    return check_launch("categorical_fisher_kernel");
}
