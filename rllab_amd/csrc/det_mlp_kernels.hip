// det_mlp_kernels.hip -- the fused rollout of a DeterministicMLPPolicy under an exploration strategy
// (rl_rollout_deterministic_mlp): the collection and the evaluation rollouts of DDPG.
//
// get_action -> step -> record -> auto-reset of rllab/algos/ddpg.py:214-246 for every env and the whole horizon in one
// launch: the per-lane horizon loop of lane_rollout.h (one wavefront per workgroup of 64 envs, every lane steps its env
// through the single-source Env::reset / step / observe, so the host build of the same headers replays the launch bit for
// bit) with the policy below.  Local to this file: the network D -> H0 -> H1 -> A at run-time widths -- staged once per
// workgroup into LDS and read at lane-uniform addresses, four units per 16-byte read, the hidden activations in this
// lane's columns of two LDS tiles -- and the two exploration rules (OUStrategy, GaussianStrategy) that stand in place of
// act = z * std + mean, the Ornstein-Uhlenbeck state in this lane's column of a third tile.  Nothing of the policy is in
// registers while an env steps, no register array is indexed at run time.
// Build with -ffp-contract=on like env_kernels.hip (the env arithmetic must match the host oracle build); the exploration
// rules are written with the single-rounding intrinsics, which that option does not fuse.
#include <hip/hip_runtime.h>
#include <math.h>
#include "../../include/rllab_amd.h"
#include "capi_util.h"
#include "device_rng.h"
#include "envs.h"
#include "gru_cell.h"
#include "lane_rollout.h"

namespace rl {

constexpr int DET_MAX_OBS = 32, DET_MAX_ACT = 8, DET_MAX_HIDDEN = 64;

// offsets (in floats) of the staged parameter vector: W0[D][H0] b0[H0] W1[H0][H1] b1[H1] W2[H1][A] b2[A], W row-major
// [in][out]; H0, H1 multiples of 4, so every row of W0 / W1 and both hidden biases start on 16 bytes
struct DetLayout {
    int b0, w1, b1, w2, b2, total;
    __host__ __device__ DetLayout(int D, int H0, int H1, int A) {
        b0 = D * H0;
        w1 = b0 + H0;
        b1 = w1 + H0 * H1;
        w2 = b1 + H1;
        b2 = w2 + H1 * A;
        total = b2 + A;
    }
};

struct DetDev : LaneRolloutDev {
    int reset_at_start, H0, H1, act_hidden, act_out, explore;
    float ou_theta, ou_mu, ou_sigma;
    float low[DET_MAX_ACT], high[DET_MAX_ACT];
    float* last_obs;
    float* explore_state;       // [Env::ACT][n], RL_EXPLORE_OU
    const float* theta;         // DetLayout
    const float* sigma_t;       // [T], RL_EXPLORE_GAUSSIAN
    uint8_t* cuts;              // [T][n] or null
};

__device__ __forceinline__ float det_activation(int code, float x) {
    if (code == RL_ACT_TANH) return tanhf(x);
    return code == RL_ACT_RECTIFY ? fmaxf(x, 0.0f) : x;
}

template <class Env>
struct DetPolicy {
    static constexpr int DO = Env::OBS, DA = Env::ACT;
    static constexpr bool RECORDS_ALL = true;
    static constexpr bool EXPLORES = true;
    static constexpr bool HEARS_ENV_DONE = true;
    const DetDev& a;
    const int i;
    const bool fresh;
    const DetLayout off;
    const LdsWeights w;
    float* h0;                  // this lane's column of the [H0][64] tile
    float* h1;                  // ... of the [H1][64] tile behind it
    float* x;                   // ... of the [DA][64] tile of Ornstein-Uhlenbeck states behind that
    int t;                      // the launch's step (wave-uniform)
    bool env_ended;

    __device__ __forceinline__ DetPolicy(const DetDev& a_, int i_, const DetLayout& off_, const float* w_, float* column)
        : a(a_), i(i_), fresh(a_.reset_at_start != 0), off(off_), w{w_}, h0(column), h1(column + a_.H0 * WV),
          x(column + (a_.H0 + a_.H1) * WV), t(0), env_ended(false) {}

    __device__ __forceinline__ void restart() {
#pragma unroll
        for (int k = 0; k < DA; ++k) x[k * WV] = a.ou_mu;
    }
    __device__ __forceinline__ void resume(float* o) {
#pragma unroll
        for (int k = 0; k < DO; ++k) o[k] = a.last_obs[(size_t)k * a.n + i];
        if (a.explore == RL_EXPLORE_OU) {
#pragma unroll
            for (int k = 0; k < DA; ++k) x[k * WV] = a.explore_state[(size_t)k * a.n + i];
        }
    }

    // per unit: acc = b[j], acc = fmaf(x[k], W[k][j], acc) for k in input order, the activation
    __device__ __forceinline__ void mean(const float* o, float* m) {
        const int H0 = a.H0, H1 = a.H1;
#pragma unroll 1
        for (int j = 0; j < H0; j += GRU_UB) {
            F4 acc = w.load4(off.b0 + j);
#pragma unroll
            for (int k = 0; k < DO; ++k) {
                const F4 q = w.load4(k * H0 + j);
#pragma unroll
                for (int u = 0; u < GRU_UB; ++u) acc.v[u] = __builtin_fmaf(o[k], q.v[u], acc.v[u]);
            }
#pragma unroll
            for (int u = 0; u < GRU_UB; ++u) h0[(j + u) * WV] = det_activation(a.act_hidden, acc.v[u]);
        }
#pragma unroll 1
        for (int j = 0; j < H1; j += GRU_UB) {
            F4 acc = w.load4(off.b1 + j);
#pragma unroll 4
            for (int k = 0; k < H0; ++k) {
                const float h = h0[k * WV];
                const F4 q = w.load4(off.w1 + k * H1 + j);
#pragma unroll
                for (int u = 0; u < GRU_UB; ++u) acc.v[u] = __builtin_fmaf(h, q.v[u], acc.v[u]);
            }
#pragma unroll
            for (int u = 0; u < GRU_UB; ++u) h1[(j + u) * WV] = det_activation(a.act_hidden, acc.v[u]);
        }
#pragma unroll
        for (int c = 0; c < DA; ++c) m[c] = w.load(off.b2 + c);
#pragma unroll 4
        for (int k = 0; k < H1; ++k) {
            const float h = h1[k * WV];
#pragma unroll
            for (int c = 0; c < DA; ++c) m[c] = __builtin_fmaf(h, w.load(off.w2 + k * DA + c), m[c]);
        }
#pragma unroll
        for (int c = 0; c < DA; ++c) m[c] = det_activation(a.act_out, m[c]);
    }

    __device__ __forceinline__ bool needs_draws() const { return a.explore != RL_EXPLORE_NONE; }
    // every operation rounded once in float32, in the order of OUStrategy.evolve_states / get_actions and of
    // GaussianStrategy.get_actions
    __device__ __forceinline__ void explore(const float* m, const float* z, float* act) {
        if (a.explore == RL_EXPLORE_OU) {
#pragma unroll
            for (int k = 0; k < DA; ++k) {
                const float xo = x[k * WV];
                const float dx = __fadd_rn(__fmul_rn(a.ou_theta, __fsub_rn(a.ou_mu, xo)), __fmul_rn(a.ou_sigma, z[k]));
                const float xn = __fadd_rn(xo, dx);
                x[k * WV] = xn;
                act[k] = fmaxf(fminf(__fadd_rn(m[k], xn), a.high[k]), a.low[k]);
            }
        } else if (a.explore == RL_EXPLORE_GAUSSIAN) {
            const float s = a.sigma_t[t];
#pragma unroll
            for (int k = 0; k < DA; ++k) act[k] = fmaxf(fminf(__fadd_rn(m[k], __fmul_rn(z[k], s)), a.high[k]), a.low[k]);
        } else {
#pragma unroll
            for (int k = 0; k < DA; ++k) act[k] = m[k];
        }
    }
    __device__ __forceinline__ void env_done(bool d) { env_ended = d; }
    // es.reset(mask=terminal): the next path starts from mu, whichever way this one ended
    __device__ __forceinline__ void stepped(const float*, float, bool d) {
        if (a.cuts) a.cuts[(size_t)t * a.n + i] = (d && !env_ended) ? 1 : 0;
        if (d) restart();
        t += 1;
    }
    __device__ __forceinline__ void finish(const float* o) {
#pragma unroll
        for (int k = 0; k < DO; ++k) a.last_obs[(size_t)k * a.n + i] = o[k];
        if (a.explore == RL_EXPLORE_OU) {
#pragma unroll
            for (int k = 0; k < DA; ++k) a.explore_state[(size_t)k * a.n + i] = x[k * WV];
        }
    }
};

// dynamic LDS: the staged parameters [w_floats], then the tiles [H0 + H1 + Env::ACT][64]
template <class Env>
__global__ void __launch_bounds__(GRU_BLOCK) rollout_det_kernel(DetDev a, int w_floats) {
    extern __shared__ __attribute__((aligned(16))) float det_smem[];
    const DetLayout off(Env::OBS, a.H0, a.H1, Env::ACT);
    for (int e = threadIdx.x; e < off.total; e += GRU_BLOCK) det_smem[e] = a.theta[e];
    __syncthreads();
    const int i = blockIdx.x * GRU_BLOCK + threadIdx.x;
    if (i >= a.n) return;                     // no cross-lane traffic from here on: the lanes past the last env just leave
    DetPolicy<Env> pol(a, i, off, det_smem, det_smem + w_floats + threadIdx.x);
    rollout_lane<Env>(a, i, pol);
}

template <class Env>
static int launch_det(const rl_det_rollout_args* g, hipStream_t st) {
    const char* entry = "rl_rollout_deterministic_mlp";
    if constexpr (Env::OBS > DET_MAX_OBS || Env::ACT > DET_MAX_ACT) {
        return set_error(RL_ERR_UNSUPPORTED, "%s: obs_dim %d, act_dim %d (at most %d and %d)", entry, (int)Env::OBS,
                         (int)Env::ACT, DET_MAX_OBS, DET_MAX_ACT);
    } else {
        DetDev a;
        int rc = lane_rollout_dev<Env>(g, g->n_envs, entry, "deterministic rollout", a);
        if (rc) return rc;
        a.reset_at_start = g->reset_at_start; a.H0 = g->hidden0; a.H1 = g->hidden1;
        a.act_hidden = g->hidden_activation; a.act_out = g->output_activation; a.explore = g->explore;
        a.ou_theta = g->ou_theta; a.ou_mu = g->ou_mu; a.ou_sigma = g->ou_sigma;
        for (int k = 0; k < DET_MAX_ACT; ++k) {
            const bool bounded = g->explore != RL_EXPLORE_NONE && k < Env::ACT;
            a.low[k] = bounded ? g->low[k] : 0.0f;
            a.high[k] = bounded ? g->high[k] : 0.0f;
        }
        a.last_obs = g->last_obs; a.explore_state = g->explore_state; a.theta = g->theta; a.sigma_t = g->sigma_t;
        a.cuts = g->cuts;
        const int w_floats = (DetLayout(Env::OBS, a.H0, a.H1, Env::ACT).total + 3) & ~3;
        const size_t lds = ((size_t)w_floats + (size_t)(a.H0 + a.H1 + Env::ACT) * WV) * sizeof(float);
        if ((double)lds > GRU_LDS_LIMIT)
            return set_error(RL_ERR_UNSUPPORTED, "%s: %zu bytes of LDS for the weights and the activation tiles (a CU has "
                                                 "160 KB)", entry, lds);
        static bool allowed = false;            // per instantiation: the widths above keep the request under 64 KB today
        if (lds > 64 * 1024)
            if (int e = allow_dynamic_lds(rollout_det_kernel<Env>, (int)GRU_LDS_LIMIT, allowed)) return e;
        const dim3 grid((unsigned)((a.n + GRU_BLOCK - 1) / GRU_BLOCK)), block(GRU_BLOCK);
        hipLaunchKernelGGL(rollout_det_kernel<Env>, grid, block, lds, st, a, w_floats);
        return check_launch("rollout_det_kernel");
    }
}

}  // namespace rl

using namespace rl;

extern "C" int rl_rollout_deterministic_mlp(const rl_det_rollout_args* g, void* stream) {
    const char* entry = "rl_rollout_deterministic_mlp";
    if (!g) return set_error(RL_ERR_ARG, "%s: null args", entry);
    if (g->n_envs <= 0 || g->horizon <= 0 || !g->state || !g->ts || !g->last_obs || !g->theta || !g->obs || !g->actions ||
        !g->means || !g->rewards || !g->dones)
        return set_error(RL_ERR_ARG, "%s: bad argument", entry);
    for (int h : {g->hidden0, g->hidden1})
        if (h < 4 || h > DET_MAX_HIDDEN || h % 4 != 0)
            return set_error(RL_ERR_ARG, "%s: hidden width %d (4 .. %d, a multiple of 4: narrower layers are padded with "
                                         "zeros)", entry, h, DET_MAX_HIDDEN);
    if (g->hidden_activation != RL_ACT_TANH && g->hidden_activation != RL_ACT_RECTIFY)
        return set_error(RL_ERR_ARG, "%s: hidden_activation %d (RL_ACT_TANH or RL_ACT_RECTIFY)", entry, g->hidden_activation);
    if (g->output_activation != RL_ACT_TANH && g->output_activation != RL_ACT_IDENTITY)
        return set_error(RL_ERR_ARG, "%s: output_activation %d (RL_ACT_TANH or RL_ACT_IDENTITY)", entry, g->output_activation);
    if (g->explore != RL_EXPLORE_NONE && g->explore != RL_EXPLORE_OU && g->explore != RL_EXPLORE_GAUSSIAN)
        return set_error(RL_ERR_ARG, "%s: explore = %d (RL_EXPLORE_NONE, RL_EXPLORE_OU or RL_EXPLORE_GAUSSIAN)", entry,
                         g->explore);
    if (g->explore != RL_EXPLORE_NONE && (!g->low || !g->high))
        return set_error(RL_ERR_ARG, "%s: exploring needs the action bounds low / high", entry);
    if (g->explore == RL_EXPLORE_OU && !g->explore_state)
        return set_error(RL_ERR_ARG, "%s: RL_EXPLORE_OU needs explore_state", entry);
    if (g->explore == RL_EXPLORE_GAUSSIAN && !g->sigma_t)
        return set_error(RL_ERR_ARG, "%s: RL_EXPLORE_GAUSSIAN needs sigma_t", entry);
    RL_DISPATCH_ENV(g->kind, launch_det<E>(g, (hipStream_t)stream))
}
