// lane_rollout.h -- the horizon loop of the kernels that keep one continuous env per lane and a per-lane policy next to it:
// get_action -> step -> record -> auto-reset for the whole horizon, made of the pieces of rollout_lane.h.  Shared by
// population_kernels.hip, gru_kernels.hip and population_gru_kernels.hip, which supply the policy.
//
// A policy is a struct with
//   static constexpr bool RECORDS_ALL   true: the five output planes are all there (the entry point checked); false: each
//                                       is stored when its pointer is set (wave-uniform tests)
//   fresh                               true: the launch starts with a reset (a constant, or a launch option)
//   restart() / resume(o)               start from the policy's initial state behind that reset / carry on from what the
//                                       previous launch saved, the observation `o` it ended on included
//   std(k)                              exp(log_std) of action k
//   mean(o, mean)                       the action mean at observation o (advances the policy's own state)
//   stepped(act, reward, done)          after the env step and its recording, ahead of the auto-reset: whatever the policy
//                                       carries from step to step (`reward` is the scaled one)
//   finish(o)                           after the last step: save what resume() reads
// and nothing of it should be alive across Env::step but what the next mean() needs.
// Optional: static constexpr bool DELAYS_ACTIONS = true and
//   delayed(act, applied)               the action the env is stepped with in place of the policy's own `act` (recorded,
//                                       and handed to stepped(), as ever); once per step, ahead of Env::step
// Optional: static constexpr bool EXPLORES = true and
//   needs_draws()                       false: the step's N(0, 1) draws z are not made (wave-uniform; z is zeros then)
//   explore(mean, z, act)               forms the action from the mean and the draws, in place of act = z * std(k) + mean
//                                       (std() is not asked for then)
// Optional: static constexpr bool HEARS_ENV_DONE = true and
//   env_done(d)                         the env's own done of this step, ahead of the cut forced at max_path_length
// A policy without the member is compiled exactly as before.
#pragma once
#include <type_traits>
#include "rollout_lane.h"

namespace rl {

template <class Policy, class = void>
struct delays_actions : std::false_type {};
template <class Policy>
struct delays_actions<Policy, std::void_t<decltype(Policy::DELAYS_ACTIONS)>> : std::bool_constant<Policy::DELAYS_ACTIONS> {};
template <class Policy, class = void>
struct explores : std::false_type {};
template <class Policy>
struct explores<Policy, std::void_t<decltype(Policy::EXPLORES)>> : std::bool_constant<Policy::EXPLORES> {};
template <class Policy, class = void>
struct hears_env_done : std::false_type {};
template <class Policy>
struct hears_env_done<Policy, std::void_t<decltype(Policy::HEARS_ENV_DONE)>> : std::bool_constant<Policy::HEARS_ENV_DONE> {};

// the by-value kernel arguments every such launch has
struct LaneRolloutDev {
    int n, T, max_path_length, normalize, env_offset;
    float scale_reward;
    uint64_t seed, step_counter;
    float* state;
    int32_t* ts;
    const float* eps;
    const float* reset_draws;
    const float* act_noise_z;
    const float* obs_noise_z;
    float* obs;
    float* actions;
    float* means;
    float* rewards;
    uint8_t* dones;
    EnvCfg cfg;
};

// the fields rl_population_args, rl_gru_rollout_args and rl_population_gru_args share by name -> LaneRolloutDev, with the
// checks all of them make
template <class Env, class Args>
static int lane_rollout_dev(const Args* g, long long n, const char* entry, const char* kernel, LaneRolloutDev& a) {
    // the widest plane [obs_dim][T][n] is addressed with size_t, a ROW of n floats with 32-bit byte offsets
    if (n > (1ll << 29)) return set_error(RL_ERR_ARG, "%s: %lld envs (at most 2^29)", entry, n);
    if (int rc = check_opts(g->opts, entry)) return rc;
    a.n = (int)n; a.T = g->horizon; a.max_path_length = g->max_path_length; a.normalize = g->normalize;
    a.env_offset = g->env_offset; a.scale_reward = g->scale_reward; a.seed = g->seed; a.step_counter = g->step_counter;
    a.state = g->state; a.ts = g->ts; a.eps = g->eps; a.reset_draws = g->reset_draws;
    a.act_noise_z = g->act_noise_z; a.obs_noise_z = g->obs_noise_z;
    a.obs = g->obs; a.actions = g->actions; a.means = g->means; a.rewards = g->rewards; a.dones = g->dones;
    int rc = device_cfg<Env>(g->cfg, a.cfg);
    if (rc) return rc;
    if constexpr (has_mjc<Env>::value) {
        // (rl_rollout_gaussian_mlp switches to its MjcEnv<Env> instantiations here: 4.7 KB of scratch per lane)
        if (a.cfg.flags & (RL_CFG_LIMIT_MUJOCO | RL_CFG_CONTACT_MUJOCO))
            return set_error(RL_ERR_UNSUPPORTED, "%s: the soft-constraint step of the legged envs (RL_CFG_LIMIT_MUJOCO / "
                                                 "RL_CFG_CONTACT_MUJOCO) is not built into the %s", entry, kernel);
    }
    return 0;
}

template <class Env, class Policy>
__device__ __forceinline__ void rollout_lane(const LaneRolloutDev& a, int i, Policy& pol) {
    constexpr int DO = Env::OBS, DA = Env::ACT;
    constexpr bool ALL = Policy::RECORDS_ALL;
    const int n = a.n, T = a.T;
    const uint32_t env_global = (uint32_t)(a.env_offset + i);
    const size_t plane = (size_t)T * n;
    float s[Env::STATE];
    load_state<Env>(a.state, n, i, s);        // persisted solver state survives a reset
    int ts = a.ts[i];
    const size_t draws_slice = (size_t)Env::RESET_DRAWS * n;
    const size_t obs_z_slice = (size_t)DO * n;
    float o[DO];
    if (pol.fresh) {
        reset_one<Env>(s, a.reset_draws, n, i, a.seed, env_global, a.step_counter, a.cfg);
        ts = 0;
        Env::template observe<float>(s, o);
        observed<Env>(o, a.cfg, a.obs_noise_z, n, i, a.seed, env_global, a.step_counter);
        pol.restart();
    } else {
        pol.resume(o);
    }

    uint32_t lane_f32 = (uint32_t)i * 4, lane_u8 = (uint32_t)i;      // byte offset of env i inside a row
    for (int t = 0; t < T; ++t) {
        const size_t off_t = (size_t)t * n + i;
        const size_t row = (size_t)t * n;
        if (ALL || a.obs) store_planes<DO>(a.obs + row, plane, lane_f32, o);
        float mean[DA], act[DA], z[DA];
        pol.mean(o, mean);
        bool draws = true;
        if constexpr (explores<Policy>::value) draws = pol.needs_draws();
        if (!draws) {
#pragma unroll
            for (int k = 0; k < DA; ++k) z[k] = 0.0f;
        } else if (a.eps) {
#pragma unroll
            for (int k = 0; k < DA; ++k) z[k] = a.eps[k * plane + off_t];
            landed<DA>(z);
        } else {
            philox_draws<DA, true>(z, a.seed, env_global, a.step_counter + (uint64_t)t, RNG_POLICY);
        }
        if constexpr (explores<Policy>::value) {
            pol.explore(mean, z, act);
        } else {
#pragma unroll
            for (int k = 0; k < DA; ++k) act[k] = __builtin_fmaf(z[k], pol.std(k), mean[k]);  // rnd * exp(log_std) + mean
        }
        if (ALL || a.actions) store_planes<DA>(a.actions + row, plane, lane_f32, act);
        if (ALL || a.means) store_planes<DA>(a.means + row, plane, lane_f32, mean);

        float r;
        bool d;
        if constexpr (delays_actions<Policy>::value) {
            float applied[DA];
            pol.delayed(act, applied);
            step_lane<Env>(s, applied, a.normalize, a.cfg,
                          a.act_noise_z ? a.act_noise_z + (size_t)t * DA * n : nullptr, n, i, a.seed, env_global,
                          a.step_counter + (uint64_t)t, o, r, d);
        } else {
            step_lane<Env>(s, act, a.normalize, a.cfg,
                          a.act_noise_z ? a.act_noise_z + (size_t)t * DA * n : nullptr, n, i, a.seed, env_global,
                          a.step_counter + (uint64_t)t, o, r, d);
        }
        ts += 1;
        if constexpr (hears_env_done<Policy>::value) pol.env_done(d);
        if (a.max_path_length > 0 && ts >= a.max_path_length) d = true;
        const float rs = r * a.scale_reward;
        const uint8_t db = d ? 1 : 0;
        if (ALL || a.rewards) store_planes<1>(a.rewards + row, plane, lane_f32, &rs);
        if (ALL || a.dones) store_planes<1>(a.dones + row, plane, lane_u8, &db);
        pol.stepped(act, rs, d);
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
    pol.finish(o);
}

}  // namespace rl
