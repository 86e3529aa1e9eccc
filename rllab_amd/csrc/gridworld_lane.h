// gridworld_lane.h -- the two rules of one GridWorld env step that both GridWorld rollouts apply per lane
// (gridworld_rollout_kernel in categorical_kernels.hip, gridworld_gru_rollout_kernel in categorical_gru_kernels.hip):
// the sampling rule of rllab/misc/special.py:10-19 and the transition of rllab/envs/grid_world_env.py:86-149.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rl {

constexpr int GRID_ACTIONS = 4;

// weighted_sample: idx = sum(cumsum(p) < u), min(idx, n_act - 1); the running sum in float32, index order
__device__ __forceinline__ int grid_weighted_sample(const float* p, float u) {
    float cs = p[0];
    int act = cs < u ? 1 : 0;
#pragma unroll
    for (int k = 1; k < GRID_ACTIONS; ++k) {
        cs = cs + p[k];
        act += cs < u ? 1 : 0;
    }
    return act > GRID_ACTIONS - 1 ? GRID_ACTIONS - 1 : act;
}

// p = softmax(logit) of the four actions in float32: max-subtracted, exp2, the sum in index order, one rcp.  The recurrent
// rollout records these probabilities and the recurrent update (categorical_gru_bptt_kernels.hip) evaluates them again:
// one expression, so that at unchanged parameters the two agree bit for bit.
__device__ __forceinline__ void grid_softmax(const float* logit, float* p) {
    const float m = fmaxf(fmaxf(logit[0], logit[1]), fmaxf(logit[2], logit[3]));
#pragma unroll
    for (int k = 0; k < GRID_ACTIONS; ++k) p[k] = __builtin_amdgcn_exp2f((logit[k] - m) * 1.4426950408889634f);
    const float iz = __builtin_amdgcn_rcpf(((p[0] + p[1]) + p[2]) + p[3]);
#pragma unroll
    for (int k = 0; k < GRID_ACTIONS; ++k) p[k] = p[k] * iz;
}

// get_possible_next_states / step: 0 left, 1 down, 2 right, 3 up; clipped at the border; a wall (or standing on a
// hole / the goal) leaves the state where it is.  Returns the next state; `done` / `reward` are the env's own (a hole:
// reward 0, done; the goal: reward 1, done) -- the horizon is the caller's.
__device__ __forceinline__ int grid_transition(const int8_t* __restrict__ cell, int n_row, int n_col, int s, int act,
                                               bool& done, float& reward) {
    const int x = s / n_col, y = s % n_col;
    int nx = x + (act == 1 ? 1 : (act == 3 ? -1 : 0));
    int ny = y + (act == 2 ? 1 : (act == 0 ? -1 : 0));
    nx = nx < 0 ? 0 : (nx > n_row - 1 ? n_row - 1 : nx);
    ny = ny < 0 ? 0 : (ny > n_col - 1 ? n_col - 1 : ny);
    int ns = nx * n_col + ny;
    const int here = cell[s], there = cell[ns];
    if (there == 1 || here == 2 || here == 3) ns = s;
    const int kind = cell[ns];
    done = kind == 2 || kind == 3;
    reward = kind == 3 ? 1.0f : 0.0f;
    return ns;
}

}  // namespace rl
