// categorical_gru_bptt_kernels.hip -- the TRPO / TNPG update of a CategoricalGRUPolicy on the dense [., T, N] planes of a
// recurrent GridWorld batch (rl_gru_categorical_eval / _grad / _fvp): what algos/npo.py's recurrent categorical closures
// compute through a Python scan and torch autograd.
//
// The layout is the Gaussian update's (gru_bptt_kernels.hip) on GruLayout<H, 4> without a log-std row: one env column per
// lane, one wavefront per workgroup of 64 columns, theta staged in LDS, the hidden state in [H][64] LDS tiles, sample
// s = t * n + i.  The one-hot observation and action planes arrive as INDEX planes, int32 state [T][N] and action [T][N],
// both clamped into range here; x W_x* is OneHotInput's row read (row state, then row S + action[t - 1] unless the step
// starts a path or the policy does not see its previous action).
//   forward  (cat_gru_fwd_kernel)      the rollout's own gru_cell and the rollout's own float32 softmax (grid_softmax), so
//                                      at unchanged parameters its probabilities are the recorded ones bit for bit.  The
//                                      head runs in float64 on those float32 probabilities with TINY = 1e-8 where
//                                      distributions/categorical.py has it:
//                                        lr = (p[a] + TINY) / (p_old[a] + TINY),  loss -= w lr adv,
//                                        kl += w sum_k p_old[k] (log(p_old[k] + TINY) - log(p[k] + TINY)).
//                                      For the gradient also h' of every step and the cotangent of the logits,
//                                        c p[a] ([j == a] - p[j]),  c = -w adv / ((p_old[a] + TINY) W).
//   tangent  (cat_gru_tangent_kernel)  carries dh/dtheta . v next to the stored h planes (gru_tangent_step), evaluates the
//                                      logits of the step again, leaves  w / W  H(p) (tangent logits)  as the cotangent of
//                                      the logits: H the Hessian of the per-sample KL in the new logits at new == old with
//                                      TINY kept (the formula of rl_categorical_fisher, categorical_kernels.hip).
//   backward, weight sums, finish      gru_bptt.h's, on OneHotPlanes / OneHotRows: the left operand of the W_x* sums is
//                                      (row == state) or (row == S + previous action), over ceil((DI + 1) / 32) row blocks.
// No atomics anywhere: the same bits every run.
#include <hip/hip_runtime.h>
#include "../../include/rllab_amd.h"
#include "capi_util.h"
#include "gridworld_lane.h"
#include "gru_bptt.h"

namespace rl {

constexpr double CAT_GRU_TINY = 1e-8;

// A recurrent categorical batch on its dense planes and the workspace of its update passes (the fields gru_bptt.h's
// kernels read carry BpttDev's names).
struct CatBpttDev {
    int n, T, include_action, n_states;
    size_t B;                   // T * n
    double inv_count;
    const float *theta, *v, *adv, *old_prob, *weights;
    const int32_t *state, *action;
    const uint8_t* start;
    float* prob;                // NULL, or where the forward sweep leaves its probabilities [4][B]
    double* part;
    float *hs, *dr, *du, *dc, *rdc;
    float* dmean;               // [4][B] cotangent of the logits
    float* wpart;
};

// (a caller's arrays are not trusted with an index)
__device__ __forceinline__ int clamp_index(int v, int count) { return v < 0 ? 0 : (v >= count ? count - 1 : v); }

// the two row indices of a lane's step from the int planes
template <int H>
struct OneHotPlanes {
    static constexpr int N_LS = 0;
    int S, s_idx, pa;
    static __device__ __forceinline__ int input_dim(const CatBpttDev& a) {
        return a.n_states + (a.include_action ? GRID_ACTIONS : 0);
    }
    __device__ __forceinline__ void load(const CatBpttDev& a, size_t s, bool first) {
        S = a.n_states;
        s_idx = clamp_index(a.state[s], S);
        pa = (first || !a.include_action) ? -1 : clamp_index(a.action[s - (size_t)a.n], GRID_ACTIONS);
    }
    __device__ __forceinline__ OneHotInput<H> input() const { return OneHotInput<H>(S, s_idx, pa); }
};

// row `row` of [onehot(state); onehot(previous action); 1] at sample s
struct OneHotRows {
    int S, DI;
    __device__ __forceinline__ float operator()(const CatBpttDev& a, int row, size_t s, bool st) const {
        if (row < S) return row == clamp_index(a.state[s], S) ? 1.0f : 0.0f;
        if (row < DI) return (!st && row - S == clamp_index(a.action[s - (size_t)a.n], GRID_ACTIONS)) ? 1.0f : 0.0f;
        return row == DI ? 1.0f : 0.0f;
    }
};

// GRAD = false: loss and KL sums only.  GRAD = true: also h' of every step, the cotangent of the logits and the per-lane
// sums of d loss / d b_out.
template <int H, bool GRAD>
__global__ void __launch_bounds__(GRU_BLOCK) cat_gru_fwd_kernel(CatBpttDev a, int w_floats) {
    constexpr int A = GRID_ACTIONS;
    const int DI = OneHotPlanes<H>::input_dim(a);
    const GruLayout<H, A> off(DI);
    GruLanes<H> lanes(a.theta, off.total, w_floats);
    const int i = blockIdx.x * GRU_BLOCK + threadIdx.x;
    const size_t B = a.B;
    double loss = 0.0, kl = 0.0, sw = 0.0, dls[A], dbo[A];
#pragma unroll
    for (int k = 0; k < A; ++k) { dls[k] = 0.0; dbo[k] = 0.0; }
    if (i < a.n) {
#pragma unroll 1
        for (int t = 0; t < a.T; ++t) {
            const size_t s = (size_t)t * a.n + i;
            const bool first = t == 0 || a.start[s];
            if (first) lanes.fill_h0();
            OneHotPlanes<H> step;
            step.load(a, s, first);
            float logit[A], p[A];
            gru_cell<H, A>(LdsWeights{lanes.w}, off, DI, step.input(), lanes.hc, lanes.hn, logit);
            lanes.swap();
            grid_softmax(logit, p);
            if (GRAD) {
#pragma unroll 4
                for (int k = 0; k < H; ++k) a.hs[(size_t)k * B + s] = lanes.hc[k * WV];
            }
            const int act = clamp_index(a.action[s], A);
            const double w = (double)a.weights[s], adv = (double)a.adv[s];
            double pa = 0.0, poa = 0.0, klv = 0.0;
#pragma unroll
            for (int k = 0; k < A; ++k) {
                if (a.prob) a.prob[(size_t)k * B + s] = p[k];
                const double pn = (double)p[k], po = (double)a.old_prob[(size_t)k * B + s];
                if (k == act) { pa = pn; poa = po; }
                klv += po * (log(po + CAT_GRU_TINY) - log(pn + CAT_GRU_TINY));
            }
            // a padded sample (w = 0) contributes nothing, whatever its planes hold
            if (w != 0.0) {
                loss -= w * ((pa + CAT_GRU_TINY) / (poa + CAT_GRU_TINY)) * adv;
                kl += w * klv;
                sw += w;
            }
            if (GRAD) {
                const double c = w != 0.0 ? -w * adv * a.inv_count / (poa + CAT_GRU_TINY) : 0.0;
#pragma unroll
                for (int k = 0; k < A; ++k) {
                    const double g = c * pa * ((k == act ? 1.0 : 0.0) - (double)p[k]);
                    a.dmean[(size_t)k * B + s] = (float)g;
                    dbo[k] += g;
                }
            }
        }
    }
    write_partials<A>(a, loss, kl, sw, dls, dbo);
}

// LDS: theta [P], v [P], the h_prev tile, then the two tangent tiles (GruLanes' hc / hn behind w_floats).  P is a multiple
// of 4: every term of GruLayout<H, 4>'s total is.
template <int H>
__global__ void __launch_bounds__(GRU_BLOCK) cat_gru_tangent_kernel(CatBpttDev a, int w_floats) {
    constexpr int A = GRID_ACTIONS;
    const int DI = OneHotPlanes<H>::input_dim(a);
    const GruLayout<H, A> off(DI);
    const int P = off.total;
    GruLanes<H> lanes(a.theta, P, w_floats);
    float* smem = const_cast<float*>(lanes.w);
    for (int e = threadIdx.x; e < P; e += GRU_BLOCK) smem[P + e] = a.v[e];
    __syncthreads();
    const LdsWeights th{lanes.w}, vw{lanes.w + P};
    float* hp = smem + 2 * P + threadIdx.x;               // this lane's column of the h_prev tile
    const int i = blockIdx.x * GRU_BLOCK + threadIdx.x;
    const size_t B = a.B;
    double sw = 0.0, dls[A], dbo[A];
#pragma unroll
    for (int k = 0; k < A; ++k) { dls[k] = 0.0; dbo[k] = 0.0; }
    if (i < a.n) {
#pragma unroll 1
        for (int t = 0; t < a.T; ++t) {
            const size_t s = (size_t)t * a.n + i;
            const bool first = t == 0 || a.start[s];
            if (first) {
#pragma unroll 1
                for (int k = 0; k < H; ++k) { hp[k * WV] = th.load(k); lanes.hc[k * WV] = 0.0f; }
            } else {
#pragma unroll 4
                for (int k = 0; k < H; ++k) hp[k * WV] = a.hs[(size_t)k * B + s - a.n];
            }
            OneHotPlanes<H> step;
            step.load(a, s, first);
            float tl[A], logit[A], pf[A];
#pragma unroll
            for (int k = 0; k < A; ++k) { tl[k] = vw.load(off.b_out + k); logit[k] = th.load(off.b_out + k); }
            gru_tangent_step<H, A, true>(th, vw, off, DI, step.input(), hp, lanes.hc, lanes.hn, tl, logit);
            lanes.swap();
            grid_softmax(logit, pf);
            const double w = (double)a.weights[s];
            if (w != 0.0) sw += w;
            // H tl = J^T (D dp) + G dp - p (G . dp) - (G . p) dp,  dp = J tl,  J = diag(p) - p p^T,
            // G_k = -p_k / (p_k + TINY),  D_k = p_k / (p_k + TINY)^2
            double p[A], dp[A], q[A], G[A], pv = 0.0;
#pragma unroll
            for (int k = 0; k < A; ++k) { p[k] = (double)pf[k]; pv += p[k] * (double)tl[k]; }
            double pq = 0.0, gdp = 0.0, gp = 0.0;
#pragma unroll
            for (int k = 0; k < A; ++k) {
                dp[k] = p[k] * ((double)tl[k] - pv);
                const double den = p[k] + CAT_GRU_TINY;
                G[k] = -p[k] / den;
                q[k] = p[k] / (den * den) * dp[k];
                pq += p[k] * q[k];
                gdp += G[k] * dp[k];
                gp += G[k] * p[k];
            }
            const double c = w != 0.0 ? w * a.inv_count : 0.0;
#pragma unroll
            for (int k = 0; k < A; ++k) {
                const double g = w != 0.0 ? c * (p[k] * (q[k] - pq) + G[k] * dp[k] - p[k] * gdp - gp * dp[k]) : 0.0;
                a.dmean[(size_t)k * B + s] = (float)g;
                dbo[k] += g;
            }
        }
    }
    write_partials<A>(a, 0.0, 0.0, sw, dls, dbo);
}

// ---- host ------------------------------------------------------------------------------------------------------------

// The shape's plan, or RL_ERR_UNSUPPORTED with the sentence.  Reads no pointer and calls nothing of HIP.
static int cat_bptt_plan(const char* fn, long long n, long long T, long long n_states, int hidden, int include_action,
                         BpttPlan& p) {
    if (hidden != 32 && hidden != 64)
        return set_error(RL_ERR_UNSUPPORTED, "%s: hidden = %d (the recurrent update kernels are built for 32 and 64)", fn,
                         hidden);
    const long long DI = n_states + (include_action ? GRID_ACTIONS : 0);
    // in double: exact far beyond any width that fits, so a map that does not fit an int is refused before it is one
    const double P = (double)hidden + 3.0 * ((double)DI * hidden + (double)hidden * hidden + hidden) +
                     (double)hidden * GRID_ACTIONS + GRID_ACTIONS;
    const double tile = (double)hidden * WV, fvp = 2.0 * P + 3.0 * tile, bwd = P + 5.0 * tile;
    const double need = (fvp > bwd ? fvp : bwd) * sizeof(float);
    if (need > GRU_LDS_LIMIT)
        return set_error(RL_ERR_UNSUPPORTED, "%s: %.0f bytes of LDS for the weights, the tangent vector and the state tiles "
                         "of %d hidden units on %lld inputs (a CU has 160 KB)", fn, need, hidden, DI);
    p.H = hidden; p.DO = (int)n_states; p.DA = GRID_ACTIONS; p.DI = (int)DI;
    p.P = (int)P; p.P4 = p.P;                             // a multiple of 4
    bptt_workspace(p, n, T);
    return 0;
}

template <int H>
static int cat_bptt_run(const CatBpttDev& a, const BpttPlan& p, int mode, double* out2, float* grad, hipStream_t st) {
    constexpr int A = GRID_ACTIONS;
    const auto refuse = [](double need) {
        return set_error(RL_ERR_UNSUPPORTED, "rl_gru_categorical: %zu bytes of LDS (a CU has 160 KB)", (size_t)need);
    };
    int rc;
    if (mode == 0) rc = launch_gru_lanes<cat_gru_fwd_kernel<H, false>, H, A>("cat_gru_fwd_kernel", a, a.n, p.DI, 0, st, refuse);
    else if (mode == 1) rc = launch_gru_lanes<cat_gru_fwd_kernel<H, true>, H, A>("cat_gru_fwd_kernel", a, a.n, p.DI, 0, st, refuse);
    else rc = launch_gru_lanes<cat_gru_tangent_kernel<H>, H, A>("cat_gru_tangent_kernel", a, a.n, p.DI, p.P + H * WV, st, refuse);
    if (rc) return rc;
    return bptt_run_tail<OneHotPlanes<H>, A, H>(a, p, OneHotRows{p.DO, p.DI}, 0, mode, out2, grad, st, refuse);
}

static int cat_bptt_entry(const char* fn, const rl_gru_categorical_batch* b, int mode, const float* v, double* out2,
                          float* grad, hipStream_t st) {
    if (!b) return set_error(RL_ERR_ARG, "%s: null batch", fn);
    if (b->n_envs <= 0 || b->horizon <= 0 || (long long)b->n_envs * b->horizon >= (1LL << 31) || b->n_states <= 0 ||
        b->n_act != GRID_ACTIONS || (b->include_action != 0 && b->include_action != 1) || !(b->inv_count > 0.0) ||
        !b->theta || !b->state || !b->action || !b->advantages || !b->old_prob || !b->start || !b->weights || !b->workspace ||
        (mode == 0 && !out2) || (mode == 1 && (!out2 || !grad)) || (mode == 2 && (!v || !grad)))
        return set_error(RL_ERR_ARG, "%s: bad argument (sizes, n_act = %d, include_action 0 / 1, inv_count > 0, or a null "
                         "pointer)", fn, GRID_ACTIONS);
    BpttPlan p;
    int rc = cat_bptt_plan(fn, b->n_envs, b->horizon, b->n_states, b->hidden, b->include_action, p);
    if (rc) return rc;
    if (b->workspace_bytes < p.bytes)
        return set_error(RL_ERR_ARG, "%s: workspace of %zu bytes, %zu needed", fn, b->workspace_bytes, p.bytes);
    CatBpttDev a;
    a.n = b->n_envs; a.T = b->horizon; a.include_action = b->include_action; a.n_states = b->n_states; a.B = p.B;
    a.inv_count = b->inv_count; a.theta = b->theta; a.v = v; a.adv = b->advantages; a.old_prob = b->old_prob;
    a.weights = b->weights; a.state = b->state; a.action = b->action; a.start = b->start;
    a.prob = mode == 2 ? nullptr : b->prob;
    bptt_bind_workspace(a, p, b->workspace);
    return p.H == 32 ? cat_bptt_run<32>(a, p, mode, out2, grad, st) : cat_bptt_run<64>(a, p, mode, out2, grad, st);
}

}  // namespace rl

using namespace rl;

extern "C" size_t rl_gru_categorical_workspace_bytes(int n_envs, int horizon, int n_states, int hidden, int include_action) {
    BpttPlan p;
    if (n_envs <= 0 || horizon <= 0 || (long long)n_envs * horizon >= (1LL << 31) || n_states <= 0) {
        set_error(RL_ERR_ARG, "rl_gru_categorical_workspace_bytes: bad argument");
        return 0;
    }
    return cat_bptt_plan("rl_gru_categorical_workspace_bytes", n_envs, horizon, n_states, hidden, include_action != 0, p)
               ? 0 : p.bytes;
}

extern "C" int rl_gru_categorical_eval(const rl_gru_categorical_batch* b, double* out2, void* stream) {
    return cat_bptt_entry("rl_gru_categorical_eval", b, 0, nullptr, out2, nullptr, (hipStream_t)stream);
}

extern "C" int rl_gru_categorical_grad(const rl_gru_categorical_batch* b, double* out2, float* grad, void* stream) {
    return cat_bptt_entry("rl_gru_categorical_grad", b, 1, nullptr, out2, grad, (hipStream_t)stream);
}

extern "C" int rl_gru_categorical_fvp(const rl_gru_categorical_batch* b, const float* v, float* out, void* stream) {
    return cat_bptt_entry("rl_gru_categorical_fvp", b, 2, v, nullptr, out, (hipStream_t)stream);
}
