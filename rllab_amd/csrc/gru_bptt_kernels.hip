// gru_bptt_kernels.hip -- the TRPO / TNPG update of a GaussianGRUPolicy on the dense [., T, N] planes of a recurrent batch
// (rl_gru_gaussian_eval / _grad / _fvp): what algos/npo.py's closures compute through a Python scan and torch autograd.
//
// The sweeps run like the rollout (gru_kernels.hip): one env column per lane, one wavefront per workgroup of 64 columns,
// theta staged in LDS, the hidden state in [H][64] LDS tiles.
//   forward  (gru_fwd_kernel)      t = 0 .. T-1: the rollout's own gru_cell, so at unchanged parameters its means are the
//                                  recorded ones bit for bit; per-lane float64 sums of the surrogate loss and the KL; for
//                                  the gradient also h' of every step and the cotangent of the means into the workspace.
//   tangent  (gru_tangent_kernel)  t = 0 .. T-1: carries dh/dtheta . v next to the h planes the gradient's forward sweep
//                                  left, leaves the cotangent  M (tangent mean) w / W,  M = 2 / (2 sigma^2 + 1e-8).
//   backward (gru_bwd_kernel)      t = T-1 .. 0: carries dh per lane, recomputes the gates of the step from the stored h
//                                  (gru_bptt.h: the forward pass's own bits), leaves the cotangents of the three gate
//                                  sums of every sample in the workspace.
// The backward sweep, the weight sums and the finish are gru_bptt.h's, shared with the categorical family
// (categorical_gru_bptt_kernels.hip); here they run on DensePlanes / DenseRows.
// No sweep accumulates a weight gradient: those are sums over all T * N samples of outer products
// [x; 1; h_prev] (x) [dr; du; dc]  (r * dc against h_prev for W_hc)  and  h' (x) dmean, and gru_wgrad_kernel takes them
// on v_mfma_f32_32x32x2_f32 with the SAMPLE axis as the k axis: a grid of (sample chunks) x (32 x 32 x {r, u, c} output
// tiles), one wavefront each, every chunk writing its own partial row; gru_finish_kernel adds the rows in chunk order.
// No atomics anywhere: the same bits every run.
#include <hip/hip_runtime.h>
#include "../../include/rllab_amd.h"
#include "capi_util.h"
#include "gru_bptt.h"

namespace rl {

// GRAD = false: loss and KL sums only.  GRAD = true: also h' of every step, the cotangent of the means, and the per-lane
// sums of d loss / d log_std and d loss / d b_out.
template <int DO, int DA, int H, bool GRAD>
__global__ void __launch_bounds__(GRU_BLOCK) gru_fwd_kernel(BpttDev a, int w_floats) {
    const int DI = DO + (a.include_action ? DA : 0);
    const GruLayout<H, DA> off(DI);
    GruLanes<H> lanes(a.theta, off.total + DA, w_floats);
    const int i = blockIdx.x * GRU_BLOCK + threadIdx.x;
    const size_t B = a.B;
    double loss = 0.0, kl = 0.0, sw = 0.0, dls[DA], dbo[DA], sn[DA], so[DA], sn2[DA], so2[DA], lsn[DA], lso[DA];
#pragma unroll
    for (int k = 0; k < DA; ++k) {
        dls[k] = 0.0; dbo[k] = 0.0;
        lsn[k] = (double)lanes.w[off.total + k]; lso[k] = (double)a.old_log_std[k];
        sn[k] = sigma_of(lanes.w[off.total + k]); so[k] = sigma_of(a.old_log_std[k]);
        // the squares rounded on their own: under FMA contraction  so * so - sn * sn  is not 0 at so == sn
        sn2[k] = sn[k] * sn[k];
        so2[k] = so[k] * so[k];
    }
    if (i < a.n) {
        float pa[DA];
#pragma unroll 1
        for (int t = 0; t < a.T; ++t) {
            const size_t s = (size_t)t * a.n + i;
            if (t == 0 || a.start[s]) {
                lanes.fill_h0();
#pragma unroll
                for (int k = 0; k < DA; ++k) pa[k] = 0.0f;
            }
            float o[DO], m[DA];
#pragma unroll
            for (int d = 0; d < DO; ++d) o[d] = a.obs[(size_t)d * B + s];
            gru_cell<H, DA>(LdsWeights{lanes.w}, off, DI, DenseInput<DO, DA, H>{o, pa, a.include_action != 0}, lanes.hc,
                            lanes.hn, m);
            lanes.swap();
            if (GRAD) {
#pragma unroll 4
                for (int k = 0; k < H; ++k) a.hs[(size_t)k * B + s] = lanes.hc[k * WV];
            }
            const double w = (double)a.weights[s], c = (double)a.adv[s] * w;
            double dl = 0.0, klv = 0.0, zn[DA];
#pragma unroll
            for (int k = 0; k < DA; ++k) {
                const float act = a.actions[(size_t)k * B + s], mo = a.old_means[(size_t)k * B + s];
                pa[k] = act;
                if (a.means) a.means[(size_t)k * B + s] = m[k];
                zn[k] = ((double)act - (double)m[k]) / sn[k];
                const double zo = ((double)act - (double)mo) / so[k], dm = (double)mo - (double)m[k];
                dl += (lso[k] - lsn[k]) + 0.5 * (zo * zo - zn[k] * zn[k]);
                klv += (dm * dm + (so2[k] - sn2[k])) / (2.0 * sn2[k] + 1e-8) + (lsn[k] - lso[k]);
            }
            // a padded sample (w = 0) contributes nothing, whatever its planes hold
            const double lr = w != 0.0 ? exp(dl) : 0.0;
            if (w != 0.0) { loss -= lr * c; kl += klv * w; sw += w; }
            if (GRAD) {
                const double g = -lr * c * a.inv_count;           // d loss / d log-likelihood of this sample
#pragma unroll
                for (int k = 0; k < DA; ++k) {
                    const double gm = g * zn[k] / sn[k];
                    a.dmean[(size_t)k * B + s] = (float)gm;
                    dbo[k] += gm;
                    dls[k] += g * (zn[k] * zn[k] - 1.0);
                }
            }
        }
    }
    write_partials<DA>(a, loss, kl, sw, dls, dbo);
}

// LDS: theta [P4], v [P4], the h_prev tile, then the two tangent tiles (GruLanes' hc / hn behind w_floats).
template <int DO, int DA, int H>
__global__ void __launch_bounds__(GRU_BLOCK) gru_tangent_kernel(BpttDev a, int w_floats) {
    const int DI = DO + (a.include_action ? DA : 0);
    const GruLayout<H, DA> off(DI);
    const int n_theta = off.total + DA, P4 = (n_theta + 3) & ~3;
    GruLanes<H> lanes(a.theta, n_theta, w_floats);
    float* smem = const_cast<float*>(lanes.w);
    for (int e = threadIdx.x; e < n_theta; e += GRU_BLOCK) smem[P4 + e] = a.v[e];
    __syncthreads();
    const LdsWeights th{lanes.w}, vw{lanes.w + P4};
    float* hp = smem + 2 * P4 + threadIdx.x;             // this lane's column of the h_prev tile
    const int i = blockIdx.x * GRU_BLOCK + threadIdx.x;
    const size_t B = a.B;
    double sw = 0.0, dbo[DA], dls[DA], M[DA];
#pragma unroll
    for (int k = 0; k < DA; ++k) {
        const double sg = sigma_of(lanes.w[off.total + k]);
        dbo[k] = 0.0; dls[k] = 0.0; M[k] = 2.0 / (2.0 * sg * sg + 1e-8);
    }
    if (i < a.n) {
        float pa[DA];
#pragma unroll 1
        for (int t = 0; t < a.T; ++t) {
            const size_t s = (size_t)t * a.n + i;
            if (t == 0 || a.start[s]) {
#pragma unroll 1
                for (int k = 0; k < H; ++k) { hp[k * WV] = th.load(k); lanes.hc[k * WV] = 0.0f; }
#pragma unroll
                for (int k = 0; k < DA; ++k) pa[k] = 0.0f;
            } else {
#pragma unroll 4
                for (int k = 0; k < H; ++k) hp[k * WV] = a.hs[(size_t)k * B + s - a.n];
#pragma unroll
                for (int k = 0; k < DA; ++k) pa[k] = a.actions[(size_t)k * B + s - a.n];
            }
            float o[DO], tm[DA];
#pragma unroll
            for (int d = 0; d < DO; ++d) o[d] = a.obs[(size_t)d * B + s];
#pragma unroll
            for (int k = 0; k < DA; ++k) tm[k] = vw.load(off.b_out + k);
            gru_tangent_step<H, DA, false>(th, vw, off, DI, DenseInput<DO, DA, H>{o, pa, a.include_action != 0}, hp, lanes.hc,
                                           lanes.hn, tm, nullptr);
            lanes.swap();
            const double w = (double)a.weights[s];
            if (w != 0.0) sw += w;
#pragma unroll
            for (int k = 0; k < DA; ++k) {
                const double gm = w != 0.0 ? M[k] * (double)tm[k] * w * a.inv_count : 0.0;
                a.dmean[(size_t)k * B + s] = (float)gm;
                dbo[k] += gm;
            }
        }
    }
    write_partials<DA>(a, 0.0, 0.0, sw, dls, dbo);
}

// ---- host ------------------------------------------------------------------------------------------------------------

// The shape's plan, or RL_ERR_UNSUPPORTED with the sentence.  Reads no pointer and calls nothing of HIP.
static int bptt_plan(const char* fn, long long n, long long T, int obs_dim, int act_dim, int hidden, int include_action,
                     BpttPlan& p) {
    if (hidden != 32 && hidden != 64)
        return set_error(RL_ERR_UNSUPPORTED, "%s: hidden = %d (the recurrent update kernels are built for 32 and 64)", fn,
                         hidden);
    const bool built = (obs_dim == 4 && act_dim == 1) || (obs_dim == 6 && act_dim == 1) || (obs_dim == 13 && act_dim == 2) ||
                       (obs_dim == 20 && act_dim == 6);
    if (!built)
        return set_error(RL_ERR_UNSUPPORTED, "%s: obs_dim %d / act_dim %d (the recurrent update kernels are built for "
                         "(4, 1), (6, 1), (13, 2) and (20, 6))", fn, obs_dim, act_dim);
    p.H = hidden; p.DO = obs_dim; p.DA = act_dim; p.DI = obs_dim + (include_action ? act_dim : 0);
    p.P = hidden + 3 * (p.DI * hidden + hidden * hidden + hidden) + hidden * act_dim + 2 * act_dim;
    p.P4 = (p.P + 3) & ~3;
    const size_t need = bptt_lds_bytes(hidden, p.P4);
    if ((double)need > GRU_LDS_LIMIT)
        return set_error(RL_ERR_UNSUPPORTED, "%s: %zu bytes of LDS for the weights, the tangent vector and the state tiles "
                         "of %d hidden units on %d inputs (a CU has 160 KB)", fn, need, hidden, p.DI);
    bptt_workspace(p, n, T);
    return 0;
}

template <int DO, int DA, int H>
static int bptt_run(const BpttDev& a, const BpttPlan& p, int mode, double* out2, float* grad, hipStream_t st) {
    const auto refuse = [](double need) {
        return set_error(RL_ERR_UNSUPPORTED, "rl_gru_gaussian: %zu bytes of LDS (a CU has 160 KB)", (size_t)need);
    };
    const int tile = H * WV;
    int rc;
    if (mode == 0) rc = launch_gru_lanes<gru_fwd_kernel<DO, DA, H, false>, H, DA>("gru_fwd_kernel", a, a.n, p.DI, DA, st, refuse);
    else if (mode == 1) rc = launch_gru_lanes<gru_fwd_kernel<DO, DA, H, true>, H, DA>("gru_fwd_kernel", a, a.n, p.DI, DA, st, refuse);
    else rc = launch_gru_lanes<gru_tangent_kernel<DO, DA, H>, H, DA>("gru_tangent_kernel", a, a.n, p.DI,
                                                                       DA + ((4 - (p.P & 3)) & 3) + p.P4 + tile, st, refuse);
    if (rc) return rc;
    return bptt_run_tail<DensePlanes<DO, DA, H>, DA, H>(a, p, DenseRows{DO, p.DI}, DA, mode, out2, grad, st, refuse);
}

static int bptt_entry(const char* fn, const rl_gru_batch* b, int mode, const float* v, double* out2, float* grad,
                      hipStream_t st) {
    if (!b) return set_error(RL_ERR_ARG, "%s: null batch", fn);
    if (b->n_envs <= 0 || b->horizon <= 0 || (long long)b->n_envs * b->horizon >= (1LL << 31) || b->obs_dim <= 0 ||
        b->act_dim <= 0 || (b->include_action != 0 && b->include_action != 1) || !(b->inv_count > 0.0) || !b->theta ||
        !b->obs || !b->actions || !b->advantages || !b->old_means || !b->old_log_std || !b->start || !b->weights ||
        !b->workspace || (mode == 0 && !out2) || (mode == 1 && (!out2 || !grad)) || (mode == 2 && (!v || !grad)))
        return set_error(RL_ERR_ARG, "%s: bad argument", fn);
    BpttPlan p;
    int rc = bptt_plan(fn, b->n_envs, b->horizon, b->obs_dim, b->act_dim, b->hidden, b->include_action, p);
    if (rc) return rc;
    if (b->workspace_bytes < p.bytes)
        return set_error(RL_ERR_ARG, "%s: workspace of %zu bytes, %zu needed", fn, b->workspace_bytes, p.bytes);
    BpttDev a;
    a.n = b->n_envs; a.T = b->horizon; a.include_action = b->include_action; a.B = p.B; a.inv_count = b->inv_count;
    a.theta = b->theta; a.v = v; a.obs = b->obs; a.actions = b->actions; a.adv = b->advantages;
    a.old_means = b->old_means; a.old_log_std = b->old_log_std; a.weights = b->weights; a.start = b->start;
    a.means = mode == 2 ? nullptr : b->means;
    bptt_bind_workspace(a, p, b->workspace);
#define RL_BPTT_SHAPE(DO_, DA_)                                                                     \
    if (p.DO == DO_ && p.DA == DA_)                                                                 \
        return p.H == 32 ? bptt_run<DO_, DA_, 32>(a, p, mode, out2, grad, st) : bptt_run<DO_, DA_, 64>(a, p, mode, out2, grad, st);
    RL_BPTT_SHAPE(4, 1) RL_BPTT_SHAPE(6, 1) RL_BPTT_SHAPE(13, 2) RL_BPTT_SHAPE(20, 6)
#undef RL_BPTT_SHAPE
    return set_error(RL_ERR_UNSUPPORTED, "%s: obs_dim %d / act_dim %d", fn, p.DO, p.DA);
}

}  // namespace rl

using namespace rl;

extern "C" size_t rl_gru_workspace_bytes(int n_envs, int horizon, int obs_dim, int act_dim, int hidden, int include_action) {
    BpttPlan p;
    if (n_envs <= 0 || horizon <= 0 || (long long)n_envs * horizon >= (1LL << 31) || obs_dim <= 0 || act_dim <= 0) {
        set_error(RL_ERR_ARG, "rl_gru_workspace_bytes: bad argument");
        return 0;
    }
    return bptt_plan("rl_gru_workspace_bytes", n_envs, horizon, obs_dim, act_dim, hidden, include_action != 0, p) ? 0 : p.bytes;
}

extern "C" int rl_gru_gaussian_eval(const rl_gru_batch* b, double* out2, void* stream) {
    return bptt_entry("rl_gru_gaussian_eval", b, 0, nullptr, out2, nullptr, (hipStream_t)stream);
}

extern "C" int rl_gru_gaussian_grad(const rl_gru_batch* b, double* out2, float* grad, void* stream) {
    return bptt_entry("rl_gru_gaussian_grad", b, 1, nullptr, out2, grad, (hipStream_t)stream);
}

extern "C" int rl_gru_gaussian_fvp(const rl_gru_batch* b, const float* v, float* out, void* stream) {
    return bptt_entry("rl_gru_gaussian_fvp", b, 2, v, nullptr, out, (hipStream_t)stream);
}
