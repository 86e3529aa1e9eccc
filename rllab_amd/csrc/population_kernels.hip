// population_kernels.hip -- the fused rollout with one parameter vector per env (rl_rollout_population).
//
// The inner loop of the cross-entropy method (rllab/algos/cem.py:29-56: set_param_values(candidate), rollout, return of
// the path) for a whole population in one launch.  Env-per-lane like rollout_kernel<Env, H, H, 64>: one wavefront per
// workgroup of 64 envs, every lane steps its env through the single-source Env::reset / step / observe (rollout_lane.h), so
// the host build of the same headers replays the launch bit for bit.  What differs is the policy: lane i evaluates the
// two-layer MLP of ITS candidate c = i % n_cand with plain float32 FMAs.  The population arrives transposed,
// theta_pop_T[P][n_cand], so lanes i, i + 1 read adjacent floats of one row: every weight load of the wavefront is one
// coalesced row segment (two at the wrap of i % n_cand), addressed as scalar row base + 32-bit lane offset.
//
// Registers: the hidden activations h0 live in LDS as [H][64] floats (lane l only ever touches column l: no bank conflict,
// no synchronisation), the unit loops run at run time over blocks of UB units whose accumulators are named registers --
// no register array is indexed at run time, nothing of the policy is alive while the physics runs.
// Build with -ffp-contract=on like env_kernels.hip (the env arithmetic must match the host oracle build).
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <type_traits>
#include "../../include/rllab_amd.h"
#include "capi_util.h"
#include "device_rng.h"
#include "envs.h"
#include "policy_mfma.h"
#include "rollout_lane.h"

namespace rl {

constexpr int POP_BLOCK = 64;   // one wavefront per workgroup, one env per lane
constexpr int UB = 4;           // hidden units evaluated together (independent FMA chains sharing the input reads)

struct PopulationDev {
    int n, n_cand, T, max_path_length, normalize, env_offset, ident1;
    float scale_reward, log_min_std;
    double discount;
    uint64_t seed, step_counter;
    float* state;
    int32_t* ts;
    const float* theta_T;
    const float* eps;
    const float* reset_draws;
    const float* act_noise_z;
    const float* obs_noise_z;
    float* obs;
    float* actions;
    float* means;
    float* rewards;
    uint8_t* dones;
    float* first_path;
    EnvCfg cfg;
};

// Rows of theta_pop_T read one after the other: the row address is a scalar that walks (one s_add_u32 / s_addc_u32 pair
// per row), the load is the scalar-base + 32-bit lane offset form of global_load -- the reading twin of store_planes
// (rollout_lane.h), for the same reason: P hoisted 64-bit row addresses fit no register file.
struct RowWalk {
    uintptr_t walk;
    __device__ __forceinline__ RowWalk(const float* theta_T, size_t row_bytes, int row)
        : walk(reinterpret_cast<uintptr_t>(theta_T) + (size_t)row * row_bytes) {}
    __device__ __forceinline__ float next(size_t row_bytes, uint32_t& lane_bytes) {
        typedef const __attribute__((address_space(1))) float* global_ptr;
        asm volatile("" : "+s"(walk));
        asm volatile("" : "+v"(lane_bytes));
        const float v = *reinterpret_cast<global_ptr>(walk + lane_bytes);
        walk += row_bytes;
        return v;
    }
    __device__ __forceinline__ void skip(size_t bytes) { walk += bytes; }    // (wraps for a step back: unsigned arithmetic)
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

template <class Env, int H>
__global__ void __launch_bounds__(POP_BLOCK) rollout_population_kernel(PopulationDev a) {
    __shared__ float h0_tile[H * WV];
    const int n = a.n, T = a.T;
    const int i = blockIdx.x * POP_BLOCK + threadIdx.x;
    if (i >= n) return;                       // no cross-lane traffic anywhere: the lanes past the last env just leave
    using N = Net<Env::OBS, Env::ACT, H>;
    const uint32_t env_global = (uint32_t)(a.env_offset + i);
    const size_t plane = (size_t)T * n;
    const size_t row_bytes = (size_t)a.n_cand * sizeof(float);
    uint32_t cand_bytes = (uint32_t)(i % a.n_cand) * 4;          // byte offset of this env's candidate inside a row
    float* h0 = h0_tile + threadIdx.x;

    // exp(max(log_std, log_min_std)) of this lane's candidate, rounded once from float64 (once per launch)
    float std_[Env::ACT];
    {
        RowWalk ls(a.theta_T, row_bytes, N::LSTD);
#pragma unroll
        for (int k = 0; k < Env::ACT; ++k)
            std_[k] = (float)exp((double)fmaxf(ls.next(row_bytes, cand_bytes), a.log_min_std));
    }

    float s[Env::STATE];
    load_state<Env>(a.state, n, i, s);        // persisted solver state survives the reset
    const size_t draws_slice = (size_t)Env::RESET_DRAWS * n;
    reset_one<Env>(s, a.reset_draws, n, i, a.seed, env_global, a.step_counter, a.cfg);
    int ts = 0;
    float o[Env::OBS];
    const size_t obs_z_slice = (size_t)Env::OBS * n;
    Env::template observe<float>(s, o);
    observed<Env>(o, a.cfg, a.obs_noise_z, n, i, a.seed, env_global, a.step_counter);

    // the first path of this env (cem.py:46-56: one rollout per candidate, its discounted and undiscounted return)
    float ret_disc = 0.0f, ret_undisc = 0.0f;
    double gpow = 1.0;                        // discount^t: float64, so the only float32 roundings are the sum's
    int first_len = 0;
    bool first_open = true;

    uint32_t lane_f32 = (uint32_t)i * 4, lane_u8 = (uint32_t)i;      // byte offset of env i inside a row
    for (int t = 0; t < T; ++t) {
        const size_t off = (size_t)t * n + i;
        const size_t row = (size_t)t * n;
        if (a.obs) store_planes<Env::OBS>(a.obs + row, plane, lane_f32, o);
        float mean[Env::ACT], act[Env::ACT], z[Env::ACT];
        population_forward<Env, H>(a.theta_T, row_bytes, cand_bytes, o, h0, a.ident1 != 0, mean);
        if (a.eps) {
#pragma unroll
            for (int k = 0; k < Env::ACT; ++k) z[k] = a.eps[k * plane + off];
            landed<Env::ACT>(z);
        } else {
            philox_draws<Env::ACT, true>(z, a.seed, env_global, a.step_counter + (uint64_t)t, RNG_POLICY);
        }
#pragma unroll
        for (int k = 0; k < Env::ACT; ++k) act[k] = __builtin_fmaf(z[k], std_[k], mean[k]);  // rnd * exp(log_std) + mean
        if (a.actions) store_planes<Env::ACT>(a.actions + row, plane, lane_f32, act);
        if (a.means) store_planes<Env::ACT>(a.means + row, plane, lane_f32, mean);

        float r;
        bool d;
        step_lane<Env>(s, act, a.normalize, a.cfg,
                      a.act_noise_z ? a.act_noise_z + (size_t)t * Env::ACT * n : nullptr, n, i, a.seed, env_global,
                      a.step_counter + (uint64_t)t, o, r, d);
        ts += 1;
        if (a.max_path_length > 0 && ts >= a.max_path_length) d = true;
        const float rs = r * a.scale_reward;
        const uint8_t db = d ? 1 : 0;
        if (a.rewards) store_planes<1>(a.rewards + row, plane, lane_f32, &rs);
        if (a.dones) store_planes<1>(a.dones + row, plane, lane_u8, &db);
        if (first_open) {
            ret_disc = __builtin_fmaf((float)gpow, rs, ret_disc);
            ret_undisc += rs;
            gpow *= a.discount;
            first_len += 1;
            first_open = !d;
        }
        if (d) {
            const float* dr = a.reset_draws ? a.reset_draws + (size_t)(t + 1) * draws_slice : nullptr;
            reset_one<Env>(s, dr, n, i, a.seed, env_global, a.step_counter + (uint64_t)t + 1, a.cfg);
            Env::template observe<float>(s, o);
            ts = 0;
        }
        observed<Env>(o, a.cfg, a.obs_noise_z ? a.obs_noise_z + (size_t)(t + 1) * obs_z_slice : nullptr, n, i, a.seed,
                      env_global, a.step_counter + (uint64_t)t + 1);
    }
    store_state<Env>(a.state, n, i, s);
    a.ts[i] = ts;
    const float fp[3] = {ret_disc, ret_undisc, (float)first_len};
    store_planes<3>(a.first_path, (size_t)n, lane_f32, fp);
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
    const long long n = (long long)g->n_cand * g->n_evals;
    // the widest plane [obs_dim][T][n] is addressed with size_t, a ROW of n floats with 32-bit byte offsets
    if (n > (1ll << 29)) return set_error(RL_ERR_ARG, "rl_rollout_population: %lld envs (at most 2^29)", n);
    PopulationDev a;
    a.n = (int)n; a.n_cand = g->n_cand; a.T = g->horizon; a.max_path_length = g->max_path_length;
    a.normalize = g->normalize; a.env_offset = g->env_offset; a.ident1 = act1 == RL_ACT_IDENTITY ? 1 : 0;
    a.scale_reward = g->scale_reward; a.log_min_std = g->log_min_std; a.discount = g->discount;
    a.seed = g->seed; a.step_counter = g->step_counter;
    a.state = g->state; a.ts = g->ts; a.theta_T = g->theta_pop_T; a.eps = g->eps; a.reset_draws = g->reset_draws;
    a.act_noise_z = g->act_noise_z; a.obs_noise_z = g->obs_noise_z;
    a.obs = g->obs; a.actions = g->actions; a.means = g->means; a.rewards = g->rewards; a.dones = g->dones;
    a.first_path = g->first_path;
    int rc = device_cfg<Env>(g->cfg, a.cfg);
    if (rc) return rc;
    if constexpr (has_mjc<Env>::value) {
        // (rl_rollout_gaussian_mlp switches to its MjcEnv<Env> instantiations here: 4.7 KB of scratch per lane)
        if (a.cfg.flags & (RL_CFG_LIMIT_MUJOCO | RL_CFG_CONTACT_MUJOCO))
            return set_error(RL_ERR_UNSUPPORTED, "rl_rollout_population: the soft-constraint step of the legged envs "
                                                 "(RL_CFG_LIMIT_MUJOCO / RL_CFG_CONTACT_MUJOCO) is not built into the population kernel");
    }
    const dim3 grid((unsigned)((n + POP_BLOCK - 1) / POP_BLOCK)), block(POP_BLOCK);
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
