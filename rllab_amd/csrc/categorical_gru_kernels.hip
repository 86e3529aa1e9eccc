// categorical_gru_kernels.hip -- the fused GridWorld rollout of a CategoricalGRUPolicy (rl_rollout_gridworld_gru).
//
// get_action -> step -> record -> auto-reset of rllab/policies/categorical_gru_policy.py:142-172 on
// rllab/envs/grid_world_env.py:86-149 for every env and the whole horizon in one launch.  rl_rollout_gridworld samples
// from a probability table indexed by the state alone; a recurrent policy's probabilities depend on each env's hidden
// state, so here they are evaluated per env and per step inside the launch.  The shape is rollout_gru_kernel's
// (gru_kernels.hip): one env per lane, one wavefront per workgroup of 64 envs, theta staged ONCE per workgroup into LDS,
// the hidden state in two [H][64] LDS tiles that swap every step (lane l only ever touches column l), the unit loop at
// run time over blocks of four units whose accumulators are named registers.
//
// What differs is the input product: x = [onehot(s), onehot(prev_action)] is one-hot, so x W_x* is a ROW READ.  Each
// gate's sum is its bias, then row s of W_x*, then row S + prev_action of W_x* (skipped at a path start), then the hidden
// units in index order with float32 FMAs.  Those row reads are the only LDS reads at lane-varying addresses: six 16-byte
// reads per unit block next to 3 H broadcast reads of W_h*.
#include <hip/hip_runtime.h>
#include "../../include/rllab_amd.h"
#include "capi_util.h"
#include "device_rng.h"
#include "gridworld_lane.h"
#include "policy_mfma.h"

namespace rl {

constexpr int GGRU_BLOCK = 64;   // one wavefront per workgroup, one env per lane
constexpr int GGRU_UB = 4;       // hidden units evaluated together: one 16-byte weight read per gate and input row
constexpr size_t GGRU_LDS_LIMIT = 160 * 1024;

// offsets (in floats) of the parameter vector for input width DI = S (+ 4): h0, then per gate W_x [DI][H], W_h [H][H],
// b [H] for r, u, c, then W_out [H][4], b_out [4] -- GruOffsets of gru_kernels.hip without the log-std row
template <int H>
struct GridGruOffsets {
    int gate, w_out, b_out, total;
    __host__ __device__ explicit GridGruOffsets(int DI) {
        gate = DI * H + H * H + H;
        w_out = H + 3 * gate;
        b_out = w_out + H * GRID_ACTIONS;
        total = b_out + GRID_ACTIONS;
    }
    __host__ __device__ int wx(int g) const { return H + g * gate; }
    __host__ __device__ int wh(int g, int DI) const { return wx(g) + DI * H; }
    __host__ __device__ int b(int g, int DI) const { return wh(g, DI) + H * H; }
};

__device__ __forceinline__ float ggru_sigmoid(float z) {       // 1 / (1 + exp(-z))
    return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(z * -1.4426950408889634f));
}

struct G4 { float v[GGRU_UB]; };
__device__ __forceinline__ G4 ggru_lds4(const float* p) {      // 16-byte aligned by construction: every row is H floats
    const float4 q = *reinterpret_cast<const float4*>(p);
    return G4{{q.x, q.y, q.z, q.w}};
}
__device__ __forceinline__ void ggru_add(G4& a, const G4& b) {
#pragma unroll
    for (int u = 0; u < GGRU_UB; ++u) a.v[u] = a.v[u] + b.v[u];
}

// one GRU step of this lane on x = [onehot(s), onehot(pa)] (pa < 0: no previous action): reads h from column `hc`,
// writes h' into column `hn`, returns the four logits
template <int H>
__device__ __forceinline__ void grid_gru_step(const float* w, int DI, int S, int s, int pa, const float* hc, float* hn,
                                              float* logit) {
    static_assert(H % GGRU_UB == 0, "unit blocks");
    const GridGruOffsets<H> off(DI);
#pragma unroll
    for (int k = 0; k < GRID_ACTIONS; ++k) logit[k] = w[off.b_out + k];
    const float* xr = w + off.wx(0); const float* hr = w + off.wh(0, DI); const float* br = w + off.b(0, DI);
    const float* xu = w + off.wx(1); const float* hu = w + off.wh(1, DI); const float* bu = w + off.b(1, DI);
    const float* xc = w + off.wx(2); const float* hcw = w + off.wh(2, DI); const float* bc = w + off.b(2, DI);
    const float* wo = w + off.w_out;
    const int row_s = s * H;
    const int row_a = (S + (pa < 0 ? 0 : pa)) * H;     // only read when pa >= 0 (then S + pa < DI)
#pragma unroll 1
    for (int j = 0; j < H; j += GGRU_UB) {
        G4 ar = ggru_lds4(br + j), au = ggru_lds4(bu + j), ax = ggru_lds4(bc + j), ah = G4{{0.0f, 0.0f, 0.0f, 0.0f}};
        ggru_add(ar, ggru_lds4(xr + row_s + j));
        ggru_add(au, ggru_lds4(xu + row_s + j));
        ggru_add(ax, ggru_lds4(xc + row_s + j));
        if (pa >= 0) {
            ggru_add(ar, ggru_lds4(xr + row_a + j));
            ggru_add(au, ggru_lds4(xu + row_a + j));
            ggru_add(ax, ggru_lds4(xc + row_a + j));
        }
#pragma unroll 8
        for (int k = 0; k < H; ++k) {
            const float h = hc[k * WV];
            const G4 wr = ggru_lds4(hr + k * H + j), wu = ggru_lds4(hu + k * H + j), wc = ggru_lds4(hcw + k * H + j);
#pragma unroll
            for (int u = 0; u < GGRU_UB; ++u) {
                ar.v[u] = __builtin_fmaf(h, wr.v[u], ar.v[u]);
                au.v[u] = __builtin_fmaf(h, wu.v[u], au.v[u]);
                ah.v[u] = __builtin_fmaf(h, wc.v[u], ah.v[u]);
            }
        }
#pragma unroll
        for (int u = 0; u < GGRU_UB; ++u) {
            const float r = ggru_sigmoid(ar.v[u]), g = ggru_sigmoid(au.v[u]);
            const float c = ftanh(__builtin_fmaf(r, ah.v[u], ax.v[u]));
            const float h_old = hc[(j + u) * WV];
            const float h_new = __builtin_fmaf(g, c, (1.0f - g) * h_old);
            hn[(j + u) * WV] = h_new;
            const G4 o = ggru_lds4(wo + (j + u) * GRID_ACTIONS);
#pragma unroll
            for (int k = 0; k < GRID_ACTIONS; ++k) logit[k] = __builtin_fmaf(h_new, o.v[k], logit[k]);
        }
    }
}

template <int H>
__global__ void __launch_bounds__(GGRU_BLOCK) gridworld_gru_rollout_kernel(rl_gridworld_gru_args a, int w_floats) {
    extern __shared__ __attribute__((aligned(16))) float ggru_smem[];
    const int S = a.n_row * a.n_col;
    const bool include_action = a.include_action != 0;
    const int DI = S + (include_action ? GRID_ACTIONS : 0);
    const GridGruOffsets<H> off(DI);
    float* w = ggru_smem;                              // [w_floats >= off.total, a multiple of 4]
    float* tile0 = ggru_smem + w_floats;               // [H][64]
    float* tile1 = tile0 + H * WV;
    for (int e = threadIdx.x; e < off.total; e += GGRU_BLOCK) w[e] = a.theta[e];
    __syncthreads();
    const int n = a.n_envs, T = a.horizon;
    const int i = blockIdx.x * GGRU_BLOCK + threadIdx.x;
    if (i >= n) return;                       // no cross-lane traffic from here on: the lanes past the last env just leave
    const uint32_t env_global = (uint32_t)(a.env_offset + i);
    float* hc = tile0 + threadIdx.x;
    float* hn = tile1 + threadIdx.x;

    int s, ts, pa;
    if (a.reset_at_start) {
        s = a.start_state;
        ts = 0;
        pa = -1;
#pragma unroll 1
        for (int k = 0; k < H; ++k) hc[k * WV] = w[k];                       // h0
    } else {
        // a continuation carries on from the state, step count, hidden state and previous action the previous launch ended on
        s = a.state[i];
        ts = a.ts[i];
        pa = a.prev_action[i];
        s = s < 0 ? 0 : (s >= S ? S - 1 : s);          // (a caller's arrays are not trusted with an index)
        pa = pa < 0 ? -1 : (pa > GRID_ACTIONS - 1 ? GRID_ACTIONS - 1 : pa);
#pragma unroll 1
        for (int k = 0; k < H; ++k) hc[k * WV] = a.hidden_state[(size_t)k * n + i];
    }

    for (int t = 0; t < T; ++t) {
        const size_t col = (size_t)t * n + i;
        for (int k = 0; k < S; ++k) a.obs[((size_t)k * T + t) * n + i] = (k == s) ? 1.0f : 0.0f;
        float logit[GRID_ACTIONS], p[GRID_ACTIONS];
        grid_gru_step<H>(w, DI, S, s, include_action ? pa : -1, hc, hn, logit);
        { float* sw = hc; hc = hn; hn = sw; }                         // hc: h of this step, what the next one reads
        // max-subtracted float32 softmax, the sum in index order
        const float m = fmaxf(fmaxf(logit[0], logit[1]), fmaxf(logit[2], logit[3]));
#pragma unroll
        for (int k = 0; k < GRID_ACTIONS; ++k) p[k] = __builtin_amdgcn_exp2f((logit[k] - m) * 1.4426950408889634f);
        const float iz = __builtin_amdgcn_rcpf(((p[0] + p[1]) + p[2]) + p[3]);
#pragma unroll
        for (int k = 0; k < GRID_ACTIONS; ++k) p[k] = p[k] * iz;
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
#pragma unroll 1
            for (int k = 0; k < H; ++k) hc[k * WV] = w[k];
        } else {
            s = ns;
            pa = act;
        }
    }
    a.state[i] = s;
    a.ts[i] = ts;
    a.prev_action[i] = pa;
#pragma unroll 1
    for (int k = 0; k < H; ++k) a.hidden_state[(size_t)k * n + i] = hc[k * WV];
}

template <int H>
static int launch_grid_gru_h(const rl_gridworld_gru_args& a, hipStream_t st) {
    const long long S = (long long)a.n_row * a.n_col;
    const long long DI = S + (a.include_action ? GRID_ACTIONS : 0);
    // (in double: exact up to 2^53, and a map of 2^31 x 2^31 cells does not wrap the count before it is refused)
    const double need = ((double)H + 3.0 * ((double)DI * H + (double)H * H + H) + (double)H * GRID_ACTIONS + GRID_ACTIONS +
                         2.0 * H * WV) * sizeof(float);
    if (need > (double)GGRU_LDS_LIMIT)
        return set_error(RL_ERR_UNSUPPORTED, "rl_rollout_gridworld_gru: %.0f bytes of LDS for the weights of a %d x %d map "
                                             "and the hidden state at hidden = %d (a CU has 160 KB)", need, a.n_row, a.n_col, H);
    const int w_floats = (GridGruOffsets<H>((int)DI).total + 3) & ~3;
    const size_t lds = ((size_t)w_floats + 2 * (size_t)H * WV) * sizeof(float);
    auto kern = gridworld_gru_rollout_kernel<H>;
    static size_t attr_lds = 0;                 // per instantiation: the largest map once asked for
    if (lds > attr_lds) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)lds);
        if (e != hipSuccess) return set_error(RL_ERR_HIP, "hipFuncSetAttribute: %s", hipGetErrorString(e));
        attr_lds = lds;
    }
    const dim3 grid((unsigned)((a.n_envs + GGRU_BLOCK - 1) / GGRU_BLOCK)), block(GGRU_BLOCK);
    hipLaunchKernelGGL(kern, grid, block, lds, st, a, w_floats);
    return check_launch("gridworld_gru_rollout_kernel");
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
