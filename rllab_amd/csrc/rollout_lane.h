// rollout_lane.h -- the per-lane pieces every env-per-lane kernel is made of: state planes in and out, reset and noise
// draws (injected planes or the Philox streams), the observed observation, one Env::step under the launch's options, the
// walking plane store, and the host-side check of an rl_env_cfg.  Shared by env_kernels.hip and lane_rollout.h (the horizon
// loop of population_kernels.hip and gru_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>
#include "../../include/rllab_amd.h"
#include "capi_util.h"
#include "device_rng.h"
#include "envs.h"

namespace rl {

template <class Env>
__device__ __forceinline__ void load_state(const float* __restrict__ state, int n, int i, float* s) {
#pragma unroll
    for (int k = 0; k < Env::STATE; ++k) s[k] = state[(size_t)k * n + i];
}
template <class Env>
__device__ __forceinline__ void store_state(float* __restrict__ state, int n, int i, const float* s) {
#pragma unroll
    for (int k = 0; k < Env::STATE; ++k) state[(size_t)k * n + i] = s[k];
}

// Values just loaded from global memory inside a wave-uniform branch are made to ARRIVE inside that branch.  The memory
// counter (vmcnt) counts loads and stores alike and the compiler places the wait at the first use: behind the join that
// is a conservative vmcnt(0) on EVERY path -- in the rollout loops it stood behind the step's trajectory stores and
// exposed their full round trip every env-step (injected noise / reset planes are the parity runs' path; a training
// run takes the other side of these branches and must not wait at all).
template <int COUNT>
__device__ __forceinline__ void landed(float* v) {
#pragma unroll
    for (int k = 0; k < COUNT; ++k) asm volatile("" : "+v"(v[k]));
}

template <class Env>
__device__ __forceinline__ void reset_one(float* s, const float* __restrict__ draws, int n, int i,
                                          uint64_t seed, uint32_t env_global, uint64_t step, const EnvCfg& cfg) {
    float d[Env::RESET_DRAWS];
    if (draws) {
#pragma unroll
        for (int k = 0; k < Env::RESET_DRAWS; ++k) d[k] = draws[(size_t)k * n + i];
        landed<Env::RESET_DRAWS>(d);
    } else {
        philox_draws<Env::RESET_DRAWS, Env::RESET_NORMAL>(d, seed, env_global, step, RNG_RESET);
    }
    Env::template reset<float>(s, d, cfg.flags, cfg.link_len);
}

// N(0,1) draws of one env for one transition: slice `z` (a [COUNT][n] plane set injected by the caller -- parity
// runs) or the Philox stream under `purpose`
template <int COUNT>
__device__ __forceinline__ void noise_draws(float* d, const float* __restrict__ z, int n, int i, uint64_t seed,
                                            uint32_t env_global, uint64_t step, uint32_t purpose) {
    if (z) {
#pragma unroll
        for (int k = 0; k < COUNT; ++k) d[k] = z[(size_t)k * n + i];
        landed<COUNT>(d);
    } else {
        philox_draws<COUNT, true>(d, seed, env_global, step, purpose);
    }
}
// the observation a caller sees: raw observation + obs_noise * N(0,1) (Box2DEnv.get_current_obs, box2d_env.py:210-218).
// Wave-uniform branch: a launch without obs noise pays one scalar compare.
template <class Env>
__device__ __forceinline__ void observed(float* o, const EnvCfg& cfg, const float* __restrict__ z, int n, int i,
                                         uint64_t seed, uint32_t env_global, uint64_t step) {
    if (cfg.obs_noise != 0.0f) {
        float zn[Env::OBS];
        noise_draws<Env::OBS>(zn, z, n, i, seed, env_global, step, RNG_OBS_NOISE);
        add_obs_noise<Env, float>(cfg, zn, o);
    }
}
// Env.step with the launch's options; draws its action-noise variates only when the option is on
template <class Env>
__device__ __forceinline__ void step_one(float* s, const float* a, int normalize, const EnvCfg& cfg,
                                         const float* __restrict__ z, int n, int i, uint64_t seed, uint32_t env_global,
                                         uint64_t step, float* o, float& r, bool& d) {
    float zn[Env::ACT];
    if (cfg.action_noise != 0.0f) noise_draws<Env::ACT>(zn, z, n, i, seed, env_global, step, RNG_ACT_NOISE);
    step_cfg<Env, float>(s, a, normalize, cfg, zn, o, r, d);
}

// Env.step with the launch's options for the kernels that keep one env per lane and a per-lane policy next to it
// (lane_rollout.h): step_one with the perturbation array ALWAYS handed to Env::step.
// step_cfg passes "no action noise" as a null pointer, and an array that is either null or live is addressed through
// memory: the 4 * ACT + 4 bytes of scratch every env-per-lane kernel reports.  Here the array is always live and holds
// -0.0f when the option is off -- the additive identity of IEEE addition for EVERY x, the zeros of either sign included
// (x + -0 = x), so `applied = act + dact[k]` is `applied = act` bit for bit, and the clamps behind it see the value
// they would have seen -- and stays in registers.  With the option on: the draws and perturbation of step_one / step_cfg.
template <class Env>
__device__ __forceinline__ void step_lane(float* s, const float* a, int normalize, const EnvCfg& cfg,
                                          const float* __restrict__ z, int n, int i, uint64_t seed, uint32_t env_global,
                                          uint64_t step, float* o, float& r, bool& d) {
    StepOpts<float> opts = opts_from_cfg<float>(cfg);
    float dact[Env::ACT];
    if (cfg.action_noise != 0.0f) {
        float zn[Env::ACT];
        noise_draws<Env::ACT>(zn, z, n, i, seed, env_global, step, RNG_ACT_NOISE);
        action_perturbation<Env, float>(cfg, zn, dact);
    } else {
#pragma unroll
        for (int k = 0; k < Env::ACT; ++k) dact[k] = -0.0f;
    }
    opts.dact = dact;
    Env::template step<float>(s, a, normalize, o, r, d, opts);
}

// v[0..NP) -> NP planes of a [NP][T][n] array at (t, i): the scalar row pointer walks the planes (one s_add_u32 /
// s_addc_u32 pair per plane), every store is the scalar-base + 32-bit lane offset form of global_store.  The asm
// statements emit nothing: they keep the walk a walk (NP hoisted 64-bit plane bases do not fit the scalar register
// file next to the argument block and come back as v_readlane reloads + vector address adds) and the zero-extension
// of the lane offset next to its add, which is what the back-end's scalar-base addressing pattern needs.
template <int NP, typename V>
__device__ __forceinline__ void store_planes(V* row_ptr, size_t plane, uint32_t& lane_bytes, const V* v) {
    typedef __attribute__((address_space(1))) V* global_ptr;
    uintptr_t walk = reinterpret_cast<uintptr_t>(row_ptr);          // address of plane k's row, a scalar
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        asm volatile("" : "+s"(walk));
        asm volatile("" : "+v"(lane_bytes));
        *reinterpret_cast<global_ptr>(walk + lane_bytes) = v[k];
        walk += plane * sizeof(V);
    }
}

// rl_env_cfg (host, may be null = the env's defaults) -> the by-value kernel argument.  frame_skip 0 = env default.
template <class Env>
static int device_cfg(const rl_env_cfg* cfg, EnvCfg& c) {
    c = default_cfg<Env, float>();
    if (!cfg) return 0;
    if (cfg->frame_skip < 0 || cfg->frame_skip > 64)
        return set_error(RL_ERR_ARG, "rl_env_cfg.frame_skip = %d (0 = env default, 1..64)", cfg->frame_skip);
    if (cfg->action_noise < 0.0f || cfg->obs_noise < 0.0f)
        return set_error(RL_ERR_ARG, "rl_env_cfg: negative noise scale");
    c.ctrl_cost_coeff = cfg->ctrl_cost_coeff; c.alive_coeff = cfg->alive_coeff;
    c.action_noise = cfg->action_noise; c.obs_noise = cfg->obs_noise;
    if (cfg->frame_skip > 0) c.frame_skip = cfg->frame_skip;
    c.flags = cfg->flags;
    constexpr bool legged = has_mjc<Env>::value;          // HalfCheetah, Walker2D, Hopper (csrc/dyn_mjc.h)
    if ((cfg->flags & RL_CFG_LIMIT_MUJOCO) && !(std::is_same<Env, Swimmer>::value || legged))
        return set_error(RL_ERR_UNSUPPORTED, "rl_env_cfg.flags: RL_CFG_LIMIT_MUJOCO (soft-constraint joint limits) is built "
                                             "for the Swimmer, HalfCheetah, Walker2D and Hopper");
    if ((cfg->flags & RL_CFG_CONTACT_MUJOCO) && !legged)
        return set_error(RL_ERR_UNSUPPORTED, "rl_env_cfg.flags: RL_CFG_CONTACT_MUJOCO (soft-constraint floor contacts) is "
                                             "built for HalfCheetah, Walker2D and Hopper");
    if (cfg->link_len < 0.0f || cfg->link_len > 8.0f)
        return set_error(RL_ERR_ARG, "rl_env_cfg.link_len = %g (0 = the model's, else (0, 8])", (double)cfg->link_len);
    if (cfg->link_len > 0.0f) c.link_len = cfg->link_len;
    return 0;
}

}  // namespace rl

// `return CALL` with E = the env type of `kind` (an extern "C" entry point's last statement)
#define RL_DISPATCH_ENV(kind, CALL)                                                         \
    switch (kind) {                                                                         \
        case RL_ENV_CARTPOLE: { using E = rl::Cartpole; return CALL; }                      \
        RL_EXTRA_ENV_CASES(CALL)                                                            \
        default: return set_error(RL_ERR_ARG, "unknown or unbuilt env kind %d", (int)(kind)); \
    }
