// categorical_gru_kernels.hip -- the fused GridWorld rollout of a CategoricalGRUPolicy (rl_rollout_gridworld_gru).
//
// get_action -> step -> record -> auto-reset of rllab/policies/categorical_gru_policy.py:142-172 on
// rllab/envs/grid_world_env.py:86-149 for every env and the whole horizon in one launch.  rl_rollout_gridworld samples
// from a probability table indexed by the state alone; a recurrent policy's probabilities depend on each env's hidden
// state, so here they are evaluated per env and per step inside the launch: one env per lane, one wavefront per workgroup
// of 64 envs, the GRU step, its parameter layout, the staged weights and the two hidden-state tiles of gru_cell.h.
//
// Local to this file: the horizon loop over the integer state machine of gridworld_lane.h and the sampling (the softmax
// is gridworld_lane.h's grid_softmax, which the update kernels of categorical_gru_bptt_kernels.hip evaluate too).
// The input x = [onehot(s), onehot(prev_action)] is one-hot, so x W_x* is a ROW READ (OneHotInput): each gate's sum is its
// bias, then row s of W_x*, then row S + prev_action of W_x* (skipped at a path start), then the hidden units in index
// order with float32 FMAs -- six 16-byte reads at lane-varying addresses per unit block next to 3 H broadcast reads of W_h*.
#include <hip/hip_runtime.h>
#include "../../include/rllab_amd.h"
#include "capi_util.h"
#include "device_rng.h"
#include "gridworld_lane.h"
#include "gru_cell.h"

namespace rl {

template <int H>
__global__ void __launch_bounds__(GRU_BLOCK) gridworld_gru_rollout_kernel(rl_gridworld_gru_args a, int w_floats) {
    const int S = a.n_row * a.n_col;
    const bool include_action = a.include_action != 0;
    const int DI = S + (include_action ? GRID_ACTIONS : 0);
    const GruLayout<H, GRID_ACTIONS> off(DI);
    GruLanes<H> lanes(a.theta, off.total, w_floats);
    const int n = a.n_envs, T = a.horizon;
    const int i = blockIdx.x * GRU_BLOCK + threadIdx.x;
    if (i >= n) return;                       // no cross-lane traffic from here on: the lanes past the last env just leave
    const uint32_t env_global = (uint32_t)(a.env_offset + i);

    int s, ts, pa;
    if (a.reset_at_start) {
        s = a.start_state;
        ts = 0;
        pa = -1;
        lanes.fill_h0();
    } else {
        // a continuation carries on from the state, step count, hidden state and previous action the previous launch ended on
        s = a.state[i];
        ts = a.ts[i];
        pa = a.prev_action[i];
        s = s < 0 ? 0 : (s >= S ? S - 1 : s);          // (a caller's arrays are not trusted with an index)
        pa = pa < 0 ? -1 : (pa > GRID_ACTIONS - 1 ? GRID_ACTIONS - 1 : pa);
        lanes.load(a.hidden_state, n, i);
    }

    for (int t = 0; t < T; ++t) {
        const size_t col = (size_t)t * n + i;
        for (int k = 0; k < S; ++k) a.obs[((size_t)k * T + t) * n + i] = (k == s) ? 1.0f : 0.0f;
        float logit[GRID_ACTIONS], p[GRID_ACTIONS];
        gru_cell<H, GRID_ACTIONS>(LdsWeights{lanes.w}, off, DI, OneHotInput<H>(S, s, include_action ? pa : -1), lanes.hc, lanes.hn, logit);
        lanes.swap();
        grid_softmax(logit, p);
        float u;
        if (a.u) u = a.u[col];
        else philox_draws<1, false>(&u, a.seed, env_global, a.step_counter + (uint64_t)t, RNG_POLICY);
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
            // env.reset() and policy.reset(dones): the next path starts at start_state from h0 with no previous action
            s = a.start_state;
            ts = 0;
            pa = -1;
            lanes.fill_h0();
        } else {
            s = ns;
            pa = act;
        }
    }
    a.state[i] = s;
    a.ts[i] = ts;
    a.prev_action[i] = pa;
    lanes.store(a.hidden_state, n, i);
}

template <int H>
static int launch_grid_gru_h(const rl_gridworld_gru_args& a, hipStream_t st) {
    const long long DI = (long long)a.n_row * a.n_col + (a.include_action ? GRID_ACTIONS : 0);
    return launch_gru_lanes<gridworld_gru_rollout_kernel<H>, H, GRID_ACTIONS>(
        "gridworld_gru_rollout_kernel", a, a.n_envs, DI, 0, st, [&a](double need) {
            return set_error(RL_ERR_UNSUPPORTED, "rl_rollout_gridworld_gru: %.0f bytes of LDS for the weights of a %d x %d map "
                                                 "and the hidden state at hidden = %d (a CU has 160 KB)", need, a.n_row, a.n_col, H);
        });
}

}  // namespace rl

using namespace rl;

extern "C" int rl_rollout_gridworld_gru(const rl_gridworld_gru_args* args, void* stream) {
    if (!args) return set_error(RL_ERR_ARG, "rl_rollout_gridworld_gru: null arguments");
    const rl_gridworld_gru_args& a = *args;
    if (a.n_envs < 1 || a.horizon < 1)
        return set_error(RL_ERR_ARG, "rl_rollout_gridworld_gru: zero-sized launch (n_envs %d, horizon %d)", a.n_envs, a.horizon);
    if (a.n_act != GRID_ACTIONS)
        return set_error(RL_ERR_ARG, "rl_rollout_gridworld_gru: n_act %d (GridWorld has %d actions)", a.n_act, GRID_ACTIONS);
    if (a.include_action != 0 && a.include_action != 1)
        return set_error(RL_ERR_ARG, "rl_rollout_gridworld_gru: include_action %d (0 or 1)", a.include_action);
    if (a.n_row < 1 || a.n_col < 1) return set_error(RL_ERR_ARG, "rl_rollout_gridworld_gru: map %d x %d", a.n_row, a.n_col);
    if (a.start_state < 0 || (long long)a.start_state >= (long long)a.n_row * a.n_col)
        return set_error(RL_ERR_ARG, "rl_rollout_gridworld_gru: start_state %d outside the map", a.start_state);
    if (a.max_path_length < 0 || a.env_offset < 0)
        return set_error(RL_ERR_ARG, "rl_rollout_gridworld_gru: negative max_path_length / env_offset");
    if (!a.cell || !a.theta || !a.state || !a.ts || !a.hidden_state || !a.prev_action || !a.obs || !a.actions || !a.prob_out ||
        !a.rewards || !a.dones)
        return set_error(RL_ERR_ARG, "rl_rollout_gridworld_gru: null pointer");
    if (a.hidden == 32) return launch_grid_gru_h<32>(a, (hipStream_t)stream);
    if (a.hidden == 64) return launch_grid_gru_h<64>(a, (hipStream_t)stream);
    return set_error(RL_ERR_UNSUPPORTED, "rl_rollout_gridworld_gru: hidden = %d (the recurrent rollout is built for 32 and 64)",
                     a.hidden);
}
