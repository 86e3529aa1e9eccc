// population_gru_kernels.hip -- the fused rollout with one GaussianGRUPolicy per env (rl_rollout_population_gru).
//
// The inner loop of CEM / CMA-ES on a recurrent policy for a whole population in one launch: the per-lane horizon loop of
// lane_rollout.h (one wavefront per workgroup of 64 envs, every lane steps its env through the single-source Env::reset /
// step / observe, so the host build of the same headers replays the launch bit for bit) with the policy below.  Local to
// this file: the recurrence of gru_kernels.hip -- per lane the hidden state and the previous action, put back to h0 and to
// 0 together with the env reset -- around the shared GRU step of gru_cell.h, which here takes its weights from this lane's
// candidate c = i % n_cand (RowWeights: theta_pop_T[P][n_cand], every read of the wavefront one coalesced row segment),
// and next to it the first-path returns of population_lane.h.  Nothing is staged: a candidate is 3.7 K floats at 32 units
// on Cartpole, times 64 lanes.  LDS holds the two [H][64] hidden-state tiles only.
// Build with -ffp-contract=on like env_kernels.hip (the env arithmetic must match the host oracle build).
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include "../../include/rllab_amd.h"
#include "capi_util.h"
#include "device_rng.h"
#include "envs.h"
#include "gru_cell.h"
#include "lane_rollout.h"
#include "population_lane.h"

namespace rl {

struct PopulationGruDev : LaneRolloutDev {
    int n_cand, include_action;
    float log_min_std;
    double discount;
    const float* theta_T;       // [P][n_cand]: GruLayout<H, Env::ACT>(DI), then log_std [Env::ACT]
    float* first_path;
};

// the policy of lane_rollout.h: the GRU of candidate i % n_cand, always from a reset, and the first path of this env
template <class Env, int H>
struct PopulationGruPolicy {
    static constexpr int DO = Env::OBS, DA = Env::ACT;
    static constexpr bool RECORDS_ALL = false, fresh = true;
    const PopulationGruDev& a;
    const int DI;
    const bool include_action;
    const GruLayout<H, DA> off;
    const RowWeights w;                       // this lane's candidate
    GruTiles<H> tiles;
    float std_[DA], pa[DA];
    FirstPath first;

    __device__ __forceinline__ PopulationGruPolicy(const PopulationGruDev& a_, int i, int DI_, const GruTiles<H>& tiles_)
        : a(a_), DI(DI_), include_action(a_.include_action != 0), off(DI_),
          w{a_.theta_T, (size_t)a_.n_cand * sizeof(float), (uint32_t)(i % a_.n_cand) * 4}, tiles(tiles_) {
        // exp(max(log_std, log_min_std)) of this lane's candidate, rounded once from float64 (once per launch)
#pragma unroll
        for (int k = 0; k < DA; ++k) std_[k] = (float)exp((double)fmaxf(w.load(off.total + k), a.log_min_std));
    }
    __device__ __forceinline__ float std(int k) const { return std_[k]; }
    __device__ __forceinline__ void restart() {
        tiles.fill_h0(w);
#pragma unroll
        for (int k = 0; k < DA; ++k) pa[k] = 0.0f;
    }
    __device__ __forceinline__ void resume(float*) {}
    __device__ __forceinline__ void mean(const float* o, float* m) {
        gru_cell<H, DA>(w, off, DI, DenseInput<DO, DA, H>{o, pa, include_action}, tiles.hc, tiles.hn, m);
        tiles.swap();
    }
    // policy.reset(dones): the next path starts from the candidate's h0 with no previous action
    __device__ __forceinline__ void stepped(const float* act, float rs, bool d) {
        first.stepped(rs, d, a.discount);
        if (d) tiles.fill_h0(w);
#pragma unroll
        for (int k = 0; k < DA; ++k) pa[k] = d ? 0.0f : act[k];
    }
    __device__ __forceinline__ void finish(const float*) {}
};

template <class Env, int H>
__global__ void __launch_bounds__(GRU_BLOCK) rollout_population_gru_kernel(PopulationGruDev a) {
    __shared__ float h_tiles[2 * H * WV];
    const int i = blockIdx.x * GRU_BLOCK + threadIdx.x;
    if (i >= a.n) return;                     // no cross-lane traffic anywhere: the lanes past the last env just leave
    GruTiles<H> tiles;
    tiles.hc = h_tiles + threadIdx.x;
    tiles.hn = tiles.hc + H * WV;
    PopulationGruPolicy<Env, H> pol(a, i, Env::OBS + (a.include_action ? Env::ACT : 0), tiles);
    rollout_lane<Env>(a, i, pol);
    pol.first.store(a.first_path, a.n, i);
}

template <class Env>
static int launch_population_gru(const rl_population_gru_args* g, hipStream_t st) {
    if (g->hidden != 32 && g->hidden != 64)
        return set_error(RL_ERR_UNSUPPORTED, "rl_rollout_population_gru: hidden = %d (the recurrent population kernel is built "
                                             "for 32 and 64)", g->hidden);
    PopulationGruDev a;
    int rc = lane_rollout_dev<Env>(g, (long long)g->n_cand * g->n_evals, "rl_rollout_population_gru",
                                   "recurrent population kernel", a);
    if (rc) return rc;
    a.n_cand = g->n_cand; a.include_action = g->include_action; a.log_min_std = g->log_min_std;
    a.discount = g->discount; a.theta_T = g->theta_pop_T; a.first_path = g->first_path;
    const dim3 grid((unsigned)((a.n + GRU_BLOCK - 1) / GRU_BLOCK)), block(GRU_BLOCK);
    if (g->hidden == 32) hipLaunchKernelGGL((rollout_population_gru_kernel<Env, 32>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((rollout_population_gru_kernel<Env, 64>), grid, block, 0, st, a);
    return check_launch("rollout_population_gru_kernel");
}

}  // namespace rl

using namespace rl;

extern "C" int rl_rollout_population_gru(const rl_population_gru_args* g, void* stream) {
    if (!g) return set_error(RL_ERR_ARG, "rl_rollout_population_gru: null args");
    if (g->n_cand <= 0 || g->n_evals <= 0 || g->horizon <= 0 || !g->state || !g->ts || !g->theta_pop_T || !g->first_path ||
        (g->include_action != 0 && g->include_action != 1))
        return set_error(RL_ERR_ARG, "rl_rollout_population_gru: bad argument");
    RL_DISPATCH_ENV(g->kind, launch_population_gru<E>(g, (hipStream_t)stream))
}
