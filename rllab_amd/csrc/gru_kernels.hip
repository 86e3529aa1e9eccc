// gru_kernels.hip -- the fused rollout of a GaussianGRUPolicy (rl_rollout_gaussian_gru).
//
// get_action -> step -> record -> auto-reset of rllab/policies/gaussian_gru_policy.py:120-143 for every env and the whole
// horizon in one launch.  Env-per-lane like rollout_population_kernel<Env, H>: one wavefront per workgroup of 64 envs,
// every lane steps its env through the single-source Env::reset / step / observe (rollout_lane.h), so the host build of
// the same headers replays the launch bit for bit.  What is new is the recurrence: per lane the kernel keeps the hidden
// state h[H] and the previous action, one GRU step (rllab/core/network.py:150-155) per env step, and puts h back to h0 and
// the previous action to 0 together with the env reset.
//
// Weights: the same for every lane, staged ONCE per workgroup into LDS in the order they arrive in and read at
// lane-uniform addresses (every lane the same address: one broadcast, no bank conflict), four output units per
// 16-byte read.  The hidden state lives in LDS too, as two [H][64] tiles (lane l only ever touches column l: no bank
// conflict, no synchronisation): a step reads all of h from one tile while it writes h' into the other, then they swap.
// The unit loop runs at run time over blocks of UB units whose accumulators are named registers -- no register array is
// indexed at run time, nothing of the policy is alive while the physics runs.
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

constexpr int GRU_BLOCK = 64;   // one wavefront per workgroup, one env per lane
constexpr int GRU_UB = 4;       // hidden units evaluated together: one 16-byte weight read per gate and input

struct GruDev {
    int n, T, max_path_length, normalize, reset_at_start, include_action, env_offset;
    float scale_reward;
    uint64_t seed, step_counter;
    float* state;
    int32_t* ts;
    float* last_obs;
    float* hidden_state;
    float* prev_action;
    const float* theta;
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

// offsets (in floats) of the parameter vector for input width DI = obs_dim (+ act_dim): h0, then per gate W_x [DI][H],
// W_h [H][H], b [H] for r, u, c, then W_out [H][DA], b_out, log_std
template <int DA, int H>
struct GruOffsets {
    int gate, w_out, b_out, lstd, total;
    __host__ __device__ explicit GruOffsets(int DI) {
        gate = DI * H + H * H + H;
        w_out = H + 3 * gate;
        b_out = w_out + H * DA;
        lstd = b_out + DA;
        total = lstd + DA;
    }
    __host__ __device__ int wx(int g) const { return H + g * gate; }
    __host__ __device__ int wh(int g, int DI) const { return wx(g) + DI * H; }
    __host__ __device__ int b(int g, int DI) const { return wh(g, DI) + H * H; }
};

__device__ __forceinline__ float fsigmoid(float z) {       // 1 / (1 + exp(-z))
    return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(z * -1.4426950408889634f));
}

struct F4 { float v[GRU_UB]; };
__device__ __forceinline__ F4 lds4(const float* p) {       // 16-byte aligned by construction: every row is H floats
    const float4 q = *reinterpret_cast<const float4*>(p);
    return F4{{q.x, q.y, q.z, q.w}};
}

// one GRU step of this lane: reads h from column `hc`, writes h' into column `hn`, returns the action mean
template <class Env, int H>
__device__ __forceinline__ void gru_step(const float* w, int DI, bool include_action, const float* o, const float* pa,
                                         const float* hc, float* hn, float* mean) {
    constexpr int DO = Env::OBS, DA = Env::ACT;
    static_assert(H % GRU_UB == 0, "unit blocks");
    const GruOffsets<DA, H> off(DI);
#pragma unroll
    for (int k = 0; k < DA; ++k) mean[k] = w[off.b_out + k];
    const float* xr = w + off.wx(0); const float* hr = w + off.wh(0, DI); const float* br = w + off.b(0, DI);
    const float* xu = w + off.wx(1); const float* hu = w + off.wh(1, DI); const float* bu = w + off.b(1, DI);
    const float* xc = w + off.wx(2); const float* hcw = w + off.wh(2, DI); const float* bc = w + off.b(2, DI);
    const float* wo = w + off.w_out;
#pragma unroll 1
    for (int j = 0; j < H; j += GRU_UB) {
        F4 ar = lds4(br + j), au = lds4(bu + j), ax = lds4(bc + j), ah = F4{{0.0f, 0.0f, 0.0f, 0.0f}};
#pragma unroll
        for (int d = 0; d < DO; ++d) {
            const F4 wr = lds4(xr + d * H + j), wu = lds4(xu + d * H + j), wc = lds4(xc + d * H + j);
#pragma unroll
            for (int u = 0; u < GRU_UB; ++u) {
                ar.v[u] = __builtin_fmaf(o[d], wr.v[u], ar.v[u]);
                au.v[u] = __builtin_fmaf(o[d], wu.v[u], au.v[u]);
                ax.v[u] = __builtin_fmaf(o[d], wc.v[u], ax.v[u]);
            }
        }
        if (include_action) {
#pragma unroll
            for (int d = 0; d < DA; ++d) {
                const F4 wr = lds4(xr + (DO + d) * H + j), wu = lds4(xu + (DO + d) * H + j), wc = lds4(xc + (DO + d) * H + j);
#pragma unroll
                for (int u = 0; u < GRU_UB; ++u) {
                    ar.v[u] = __builtin_fmaf(pa[d], wr.v[u], ar.v[u]);
                    au.v[u] = __builtin_fmaf(pa[d], wu.v[u], au.v[u]);
                    ax.v[u] = __builtin_fmaf(pa[d], wc.v[u], ax.v[u]);
                }
            }
        }
#pragma unroll 8
        for (int k = 0; k < H; ++k) {
            const float h = hc[k * WV];
            const F4 wr = lds4(hr + k * H + j), wu = lds4(hu + k * H + j), wc = lds4(hcw + k * H + j);
#pragma unroll
            for (int u = 0; u < GRU_UB; ++u) {
                ar.v[u] = __builtin_fmaf(h, wr.v[u], ar.v[u]);
                au.v[u] = __builtin_fmaf(h, wu.v[u], au.v[u]);
                ah.v[u] = __builtin_fmaf(h, wc.v[u], ah.v[u]);
            }
        }
#pragma unroll
        for (int u = 0; u < GRU_UB; ++u) {
            const float r = fsigmoid(ar.v[u]), g = fsigmoid(au.v[u]);
            const float c = ftanh(__builtin_fmaf(r, ah.v[u], ax.v[u]));
            const float h_old = hc[(j + u) * WV];
            const float h_new = __builtin_fmaf(g, c, (1.0f - g) * h_old);
            hn[(j + u) * WV] = h_new;
#pragma unroll
            for (int k = 0; k < DA; ++k) mean[k] = __builtin_fmaf(h_new, wo[(j + u) * DA + k], mean[k]);
        }
    }
}

template <class Env, int H>
__global__ void __launch_bounds__(GRU_BLOCK) rollout_gru_kernel(GruDev a, int w_floats) {
    extern __shared__ __attribute__((aligned(16))) float gru_smem[];
    constexpr int DO = Env::OBS, DA = Env::ACT;
    const bool include_action = a.include_action != 0;
    const int DI = DO + (include_action ? DA : 0);
    const GruOffsets<DA, H> off(DI);
    float* w = gru_smem;                              // [w_floats >= off.total, a multiple of 4]
    float* tile0 = gru_smem + w_floats;               // [H][64]
    float* tile1 = tile0 + H * WV;
    for (int e = threadIdx.x; e < off.total; e += GRU_BLOCK) w[e] = a.theta[e];
    __syncthreads();
    const int n = a.n, T = a.T;
    const int i = blockIdx.x * GRU_BLOCK + threadIdx.x;
    if (i >= n) return;                       // no cross-lane traffic from here on: the lanes past the last env just leave
    const uint32_t env_global = (uint32_t)(a.env_offset + i);
    const size_t plane = (size_t)T * n;
    float* hc = tile0 + threadIdx.x;
    float* hn = tile1 + threadIdx.x;

    // exp(log_std), rounded once from float64 (once per launch)
    float std_[DA];
#pragma unroll
    for (int k = 0; k < DA; ++k) std_[k] = (float)exp((double)w[off.lstd + k]);

    float s[Env::STATE];
    load_state<Env>(a.state, n, i, s);
    int ts = a.ts[i];
    const size_t draws_slice = (size_t)Env::RESET_DRAWS * n;
    const size_t obs_z_slice = (size_t)Env::OBS * n;
    float o[DO], pa[DA];
    if (a.reset_at_start) {
        reset_one<Env>(s, a.reset_draws, n, i, a.seed, env_global, a.step_counter, a.cfg);
        ts = 0;
        Env::template observe<float>(s, o);
        observed<Env>(o, a.cfg, a.obs_noise_z, n, i, a.seed, env_global, a.step_counter);
#pragma unroll 1
        for (int k = 0; k < H; ++k) hc[k * WV] = w[k];                       // h0
#pragma unroll
        for (int k = 0; k < DA; ++k) pa[k] = 0.0f;
    } else {
        // a continuation carries on from the observation, hidden state and previous action the previous launch ended on
#pragma unroll
        for (int k = 0; k < DO; ++k) o[k] = a.last_obs[(size_t)k * n + i];
#pragma unroll 1
        for (int k = 0; k < H; ++k) hc[k * WV] = a.hidden_state[(size_t)k * n + i];
#pragma unroll
        for (int k = 0; k < DA; ++k) pa[k] = a.prev_action[(size_t)k * n + i];
    }

    uint32_t lane_f32 = (uint32_t)i * 4, lane_u8 = (uint32_t)i;      // byte offset of env i inside a row
    for (int t = 0; t < T; ++t) {
        const size_t off_t = (size_t)t * n + i;
        const size_t row = (size_t)t * n;
        store_planes<DO>(a.obs + row, plane, lane_f32, o);
        float mean[DA], act[DA], z[DA];
        gru_step<Env, H>(w, DI, include_action, o, pa, hc, hn, mean);
        { float* sw = hc; hc = hn; hn = sw; }                         // hc: h of this step, what the next one reads
        if (a.eps) {
#pragma unroll
            for (int k = 0; k < DA; ++k) z[k] = a.eps[k * plane + off_t];
            landed<DA>(z);
        } else {
            philox_draws<DA, true>(z, a.seed, env_global, a.step_counter + (uint64_t)t, RNG_POLICY);
        }
#pragma unroll
        for (int k = 0; k < DA; ++k) act[k] = __builtin_fmaf(z[k], std_[k], mean[k]);  // rnd * exp(log_std) + mean
        store_planes<DA>(a.actions + row, plane, lane_f32, act);
        store_planes<DA>(a.means + row, plane, lane_f32, mean);

        float r;
        bool d;
        step_lane<Env>(s, act, a.normalize, a.cfg,
                      a.act_noise_z ? a.act_noise_z + (size_t)t * DA * n : nullptr, n, i, a.seed, env_global,
                      a.step_counter + (uint64_t)t, o, r, d);
        ts += 1;
        if (a.max_path_length > 0 && ts >= a.max_path_length) d = true;
        const float rs = r * a.scale_reward;
        const uint8_t db = d ? 1 : 0;
        store_planes<1>(a.rewards + row, plane, lane_f32, &rs);
        store_planes<1>(a.dones + row, plane, lane_u8, &db);
        if (d) {
            const float* dr = a.reset_draws ? a.reset_draws + (size_t)(t + 1) * draws_slice : nullptr;
            reset_one<Env>(s, dr, n, i, a.seed, env_global, a.step_counter + (uint64_t)t + 1, a.cfg);
            Env::template observe<float>(s, o);
            ts = 0;
            // policy.reset(dones): the next path starts from h0 with no previous action
#pragma unroll 1
            for (int k = 0; k < H; ++k) hc[k * WV] = w[k];
        }
#pragma unroll
        for (int k = 0; k < DA; ++k) pa[k] = d ? 0.0f : act[k];
        observed<Env>(o, a.cfg, a.obs_noise_z ? a.obs_noise_z + (size_t)(t + 1) * obs_z_slice : nullptr, n, i, a.seed,
                      env_global, a.step_counter + (uint64_t)t + 1);
    }
    store_state<Env>(a.state, n, i, s);
    a.ts[i] = ts;
#pragma unroll
    for (int k = 0; k < DO; ++k) a.last_obs[(size_t)k * n + i] = o[k];
#pragma unroll 1
    for (int k = 0; k < H; ++k) a.hidden_state[(size_t)k * n + i] = hc[k * WV];
#pragma unroll
    for (int k = 0; k < DA; ++k) a.prev_action[(size_t)k * n + i] = pa[k];
}

template <class Env, int H>
static int launch_gru_h(const GruDev& a, hipStream_t st) {
    const int DI = Env::OBS + (a.include_action ? Env::ACT : 0);
    const int w_floats = (GruOffsets<Env::ACT, H>(DI).total + 3) & ~3;
    const size_t lds = ((size_t)w_floats + 2 * (size_t)H * WV) * sizeof(float);
    if (lds > 160 * 1024)
        return set_error(RL_ERR_UNSUPPORTED, "rl_rollout_gaussian_gru: %zu bytes of LDS for the weights and the hidden state "
                                             "(a CU has 160 KB)", lds);
    auto kern = rollout_gru_kernel<Env, H>;
    static size_t attr_lds = 0;                 // per instantiation: the larger of the two input widths once asked for
    if (lds > attr_lds) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)lds);
        if (e != hipSuccess) return set_error(RL_ERR_HIP, "hipFuncSetAttribute: %s", hipGetErrorString(e));
        attr_lds = lds;
    }
    const dim3 grid((unsigned)((a.n + GRU_BLOCK - 1) / GRU_BLOCK)), block(GRU_BLOCK);
    hipLaunchKernelGGL(kern, grid, block, lds, st, a, w_floats);
    return check_launch("rollout_gru_kernel");
}

template <class Env>
static int launch_gru(const rl_gru_rollout_args* g, hipStream_t st) {
    if (g->hidden != 32 && g->hidden != 64)
        return set_error(RL_ERR_UNSUPPORTED, "rl_rollout_gaussian_gru: hidden = %d (the recurrent rollout is built for 32 and 64)",
                         g->hidden);
    // the widest plane [obs_dim][T][n] is addressed with size_t, a ROW of n floats with 32-bit byte offsets
    if (g->n_envs > (1 << 29)) return set_error(RL_ERR_ARG, "rl_rollout_gaussian_gru: %d envs (at most 2^29)", g->n_envs);
    GruDev a;
    a.n = g->n_envs; a.T = g->horizon; a.max_path_length = g->max_path_length; a.normalize = g->normalize;
    a.reset_at_start = g->reset_at_start; a.include_action = g->include_action; a.env_offset = g->env_offset;
    a.scale_reward = g->scale_reward; a.seed = g->seed; a.step_counter = g->step_counter;
    a.state = g->state; a.ts = g->ts; a.last_obs = g->last_obs; a.hidden_state = g->hidden_state;
    a.prev_action = g->prev_action; a.theta = g->theta; a.eps = g->eps; a.reset_draws = g->reset_draws;
    a.act_noise_z = g->act_noise_z; a.obs_noise_z = g->obs_noise_z;
    a.obs = g->obs; a.actions = g->actions; a.means = g->means; a.rewards = g->rewards; a.dones = g->dones;
    int rc = device_cfg<Env>(g->cfg, a.cfg);
    if (rc) return rc;
    if constexpr (has_mjc<Env>::value) {
        if (a.cfg.flags & (RL_CFG_LIMIT_MUJOCO | RL_CFG_CONTACT_MUJOCO))
            return set_error(RL_ERR_UNSUPPORTED, "rl_rollout_gaussian_gru: the soft-constraint step of the legged envs "
                                                 "(RL_CFG_LIMIT_MUJOCO / RL_CFG_CONTACT_MUJOCO) is not built into the recurrent rollout");
    }
    if (g->hidden == 32) return launch_gru_h<Env, 32>(a, st);
    return launch_gru_h<Env, 64>(a, st);
}

}  // namespace rl

using namespace rl;

extern "C" int rl_rollout_gaussian_gru(const rl_gru_rollout_args* g, void* stream) {
    if (!g) return set_error(RL_ERR_ARG, "rl_rollout_gaussian_gru: null args");
    if (g->n_envs <= 0 || g->horizon <= 0 || !g->state || !g->ts || !g->last_obs || !g->hidden_state || !g->prev_action ||
        !g->theta || !g->obs || !g->actions || !g->means || !g->rewards || !g->dones ||
        (g->include_action != 0 && g->include_action != 1))
        return set_error(RL_ERR_ARG, "rl_rollout_gaussian_gru: bad argument");
    RL_DISPATCH_ENV(g->kind, launch_gru<E>(g, (hipStream_t)stream))
}
