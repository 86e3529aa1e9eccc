// gru_kernels.hip -- the fused rollout of a GaussianGRUPolicy (rl_rollout_gaussian_gru).
//
// get_action -> step -> record -> auto-reset of rllab/policies/gaussian_gru_policy.py:120-143 for every env and the whole
// horizon in one launch: the per-lane horizon loop of lane_rollout.h (one wavefront per workgroup of 64 envs, every lane
// steps its env through the single-source Env::reset / step / observe, so the host build of the same headers replays the
// launch bit for bit) with the policy below.  Local to this file: the recurrence around the shared GRU step of gru_cell.h
// -- per lane the hidden state h[H] and the previous action, put back to h0 and to 0 together with the env reset, carried
// from launch to launch in the caller's planes -- and the log-std row behind the GRU's parameters.
// Build with -ffp-contract=on like env_kernels.hip (the env arithmetic must match the host oracle build).
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include "../../include/rllab_amd.h"
#include "capi_util.h"
#include "device_rng.h"
#include "envs.h"
#include "gru_cell.h"
#include "lane_rollout.h"

namespace rl {

struct GruDev : LaneRolloutDev {
    int reset_at_start, include_action;
    float* last_obs;
    float* hidden_state;
    float* prev_action;
    const float* theta;         // GruLayout<H, Env::ACT>(DI), then log_std [Env::ACT]
};

template <class Env, int H>
struct GruPolicy {
    static constexpr int DO = Env::OBS, DA = Env::ACT;
    static constexpr bool RECORDS_ALL = true;
    const GruDev& a;
    const int i, DI;
    const bool fresh, include_action;
    const GruLayout<H, DA> off;
    GruLanes<H> lanes;
    float std_[DA], pa[DA];

    __device__ __forceinline__ GruPolicy(const GruDev& a_, int i_, int DI_, const GruLanes<H>& lanes_)
        : a(a_), i(i_), DI(DI_), fresh(a_.reset_at_start != 0), include_action(a_.include_action != 0), off(DI_),
          lanes(lanes_) {
        // exp(log_std), rounded once from float64 (once per launch)
#pragma unroll
        for (int k = 0; k < DA; ++k) std_[k] = (float)exp((double)lanes.w[off.total + k]);
    }
    __device__ __forceinline__ float std(int k) const { return std_[k]; }
    __device__ __forceinline__ void restart() {
        lanes.fill_h0();
#pragma unroll
        for (int k = 0; k < DA; ++k) pa[k] = 0.0f;
    }
    __device__ __forceinline__ void resume(float* o) {
#pragma unroll
        for (int k = 0; k < DO; ++k) o[k] = a.last_obs[(size_t)k * a.n + i];
        lanes.load(a.hidden_state, a.n, i);
#pragma unroll
        for (int k = 0; k < DA; ++k) pa[k] = a.prev_action[(size_t)k * a.n + i];
    }
    __device__ __forceinline__ void mean(const float* o, float* m) {
        gru_cell<H, DA>(LdsWeights{lanes.w}, off, DI, DenseInput<DO, DA, H>{o, pa, include_action}, lanes.hc, lanes.hn, m);
        lanes.swap();
    }
    // policy.reset(dones): the next path starts from h0 with no previous action
    __device__ __forceinline__ void stepped(const float* act, float, bool d) {
        if (d) lanes.fill_h0();
#pragma unroll
        for (int k = 0; k < DA; ++k) pa[k] = d ? 0.0f : act[k];
    }
    __device__ __forceinline__ void finish(const float* o) {
#pragma unroll
        for (int k = 0; k < DO; ++k) a.last_obs[(size_t)k * a.n + i] = o[k];
        lanes.store(a.hidden_state, a.n, i);
#pragma unroll
        for (int k = 0; k < DA; ++k) a.prev_action[(size_t)k * a.n + i] = pa[k];
    }
};

template <class Env, int H>
__global__ void __launch_bounds__(GRU_BLOCK) rollout_gru_kernel(GruDev a, int w_floats) {
    const int DI = Env::OBS + (a.include_action ? Env::ACT : 0);
    const GruLanes<H> lanes(a.theta, GruLayout<H, Env::ACT>(DI).total + Env::ACT, w_floats);
    const int i = blockIdx.x * GRU_BLOCK + threadIdx.x;
    if (i >= a.n) return;                     // no cross-lane traffic from here on: the lanes past the last env just leave
    GruPolicy<Env, H> pol(a, i, DI, lanes);
    rollout_lane<Env>(a, i, pol);
}

// -- DelayedActionEnv: the env is stepped with the action its policy chose `delay` steps earlier in the same path ---------
// The queue is this lane's column of an LDS ring [delay * DA][64] behind the two hidden tiles: slot (t % delay) holds the
// action of step t - delay (zeros before the path's step `delay`), is read at step t and overwritten with the action of
// step t.  The slot index counts up with the launch's own t on every lane alike (wave-uniform, no register array is
// indexed); a done zeroes the lane's whole column, after which any slot is as good a start as slot 0.
struct GruDelayDev : GruDev {
    int delay;
    float* action_queue;        // [delay][Env::ACT][n], oldest first
};

template <class Env, int H>
struct GruDelayPolicy : GruPolicy<Env, H> {
    using Base = GruPolicy<Env, H>;
    static constexpr int DA = Env::ACT;
    static constexpr bool DELAYS_ACTIONS = true;
    const GruDelayDev& q;
    float* ring;                // this lane's column: entry e of the ring at ring[e * WV]
    int slot;                   // t % delay: the oldest entry, the one the next step reads

    __device__ __forceinline__ GruDelayPolicy(const GruDelayDev& a_, int i_, int DI_, const GruLanes<H>& lanes_)
        : Base(a_, i_, DI_, lanes_), q(a_), ring(lanes_.hc + 2 * H * WV), slot(0) {}
    __device__ __forceinline__ void clear() {
#pragma unroll 1
        for (int e = 0; e < q.delay * DA; ++e) ring[e * WV] = 0.0f;
    }
    __device__ __forceinline__ void restart() {
        Base::restart();
        clear();
    }
    __device__ __forceinline__ void resume(float* o) {
        Base::resume(o);
#pragma unroll 1
        for (int e = 0; e < q.delay * DA; ++e) ring[e * WV] = q.action_queue[(size_t)e * q.n + this->i];
    }
    __device__ __forceinline__ void delayed(const float* act, float* applied) {
        float* p = ring + slot * (DA * WV);
#pragma unroll
        for (int k = 0; k < DA; ++k) {
            applied[k] = p[k * WV];
            p[k * WV] = act[k];
        }
        slot = slot + 1 == q.delay ? 0 : slot + 1;
    }
    // DelayedActionEnv.reset(): the next path starts with an empty queue
    __device__ __forceinline__ void stepped(const float* act, float r, bool d) {
        Base::stepped(act, r, d);
        if (d) clear();
    }
    __device__ __forceinline__ void finish(const float* o) {
        Base::finish(o);
        int src = slot;
#pragma unroll 1
        for (int j = 0; j < q.delay; ++j) {
#pragma unroll
            for (int k = 0; k < DA; ++k)
                q.action_queue[(size_t)(j * DA + k) * q.n + this->i] = ring[(src * DA + k) * WV];
            src = src + 1 == q.delay ? 0 : src + 1;
        }
    }
};

template <class Env, int H>
__global__ void __launch_bounds__(GRU_BLOCK) rollout_gru_delay_kernel(GruDelayDev a, int w_floats) {
    const int DI = Env::OBS + (a.include_action ? Env::ACT : 0);
    // w_floats counts the ring too (launch_gru_lanes' `extra`); the tiles stay right behind the staged parameters
    const int n_theta = GruLayout<H, Env::ACT>(DI).total + Env::ACT;
    const GruLanes<H> lanes(a.theta, n_theta, (n_theta + 3) & ~3);
    const int i = blockIdx.x * GRU_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    GruDelayPolicy<Env, H> pol(a, i, DI, lanes);
    rollout_lane<Env>(a, i, pol);
}

constexpr int GRU_MAX_DELAY = 16;

template <class Env>
static int launch_gru(const rl_gru_rollout_args* g, int delay, float* action_queue, hipStream_t st) {
    const char* entry = delay ? "rl_rollout_gaussian_gru_delayed" : "rl_rollout_gaussian_gru";
    if (g->hidden != 32 && g->hidden != 64)
        return set_error(RL_ERR_UNSUPPORTED, "%s: hidden = %d (the recurrent rollout is built for 32 and 64)", entry, g->hidden);
    GruDelayDev a;
    int rc = lane_rollout_dev<Env>(g, g->n_envs, entry, "recurrent rollout", a);
    if (rc) return rc;
    a.reset_at_start = g->reset_at_start; a.include_action = g->include_action;
    a.last_obs = g->last_obs; a.hidden_state = g->hidden_state; a.prev_action = g->prev_action; a.theta = g->theta;
    a.delay = delay; a.action_queue = action_queue;
    const int DI = Env::OBS + (a.include_action ? Env::ACT : 0);
    if (delay) {
        const auto refuse = [](double need) {
            return set_error(RL_ERR_UNSUPPORTED, "rl_rollout_gaussian_gru_delayed: %zu bytes of LDS for the weights, the hidden "
                                                 "state and the action queue (a CU has 160 KB)", (size_t)need);
        };
        const int extra = Env::ACT + delay * Env::ACT * WV;      // the log-std row, and the ring behind the tiles
        if (g->hidden == 32)
            return launch_gru_lanes<rollout_gru_delay_kernel<Env, 32>, 32, Env::ACT>("rollout_gru_delay_kernel", a, a.n, DI, extra,
                                                                                     st, refuse);
        return launch_gru_lanes<rollout_gru_delay_kernel<Env, 64>, 64, Env::ACT>("rollout_gru_delay_kernel", a, a.n, DI, extra, st,
                                                                                 refuse);
    }
    const GruDev& plain = a;
    const auto refuse = [](double need) {
        return set_error(RL_ERR_UNSUPPORTED, "rl_rollout_gaussian_gru: %zu bytes of LDS for the weights and the hidden state "
                                             "(a CU has 160 KB)", (size_t)need);
    };
    if (g->hidden == 32)
        return launch_gru_lanes<rollout_gru_kernel<Env, 32>, 32, Env::ACT>("rollout_gru_kernel", plain, a.n, DI, Env::ACT, st, refuse);
    return launch_gru_lanes<rollout_gru_kernel<Env, 64>, 64, Env::ACT>("rollout_gru_kernel", plain, a.n, DI, Env::ACT, st, refuse);
}

}  // namespace rl

using namespace rl;

static int gru_rollout_args_ok(const rl_gru_rollout_args* g) {
    return g->n_envs > 0 && g->horizon > 0 && g->state && g->ts && g->last_obs && g->hidden_state && g->prev_action &&
           g->theta && g->obs && g->actions && g->means && g->rewards && g->dones &&
           (g->include_action == 0 || g->include_action == 1);
}

extern "C" int rl_rollout_gaussian_gru(const rl_gru_rollout_args* g, void* stream) {
    if (!g) return set_error(RL_ERR_ARG, "rl_rollout_gaussian_gru: null args");
    if (!gru_rollout_args_ok(g)) return set_error(RL_ERR_ARG, "rl_rollout_gaussian_gru: bad argument");
    RL_DISPATCH_ENV(g->kind, launch_gru<E>(g, 0, nullptr, (hipStream_t)stream))
}

extern "C" int rl_rollout_gaussian_gru_delayed(const rl_gru_rollout_args* g, int32_t action_delay, float* action_queue,
                                               void* stream) {
    if (!g) return set_error(RL_ERR_ARG, "rl_rollout_gaussian_gru_delayed: null args");
    if (!gru_rollout_args_ok(g) || !action_queue)
        return set_error(RL_ERR_ARG, "rl_rollout_gaussian_gru_delayed: bad argument");
    if (action_delay < 1 || action_delay > GRU_MAX_DELAY)
        return set_error(RL_ERR_ARG, "rl_rollout_gaussian_gru_delayed: action_delay = %d (1 .. %d)", (int)action_delay,
                         GRU_MAX_DELAY);
    RL_DISPATCH_ENV(g->kind, launch_gru<E>(g, action_delay, action_queue, (hipStream_t)stream))
}
