// ddpg_kernels.hip -- K whole DDPG updates (rllab/algos/ddpg.py:331-365) in ONE launch of ONE workgroup.
//
// An update at the reference's size (batch 32, (32, 32) networks) is a few hundred thousand FMAs behind dozens of
// launches in any framework, and update u + 1 reads what update u wrote: the launches cannot overlap.  Here the
// workgroup loads the parameters once, keeps them in LDS for all K updates and writes them back at the end.
//
// One update, in the reference's order (f_train_qf, f_train_policy, then the targets):
//   1. batch      rows of the replay pool: args.indices, or Philox draws (dd_draw_row)
//   2. targets    a' = mu_targ(s'), q' = Q_targ(s', a'), y = r + (1 - term) discount q'
//   3. Q step     q = Q(s, a), loss = mean((y - q)^2) + 0.5 wd sum ||W||^2, one Adam / SGD step on theta_Q
//   4. pi step    surr = -mean(Q(s, mu(s))) at the theta_Q step 3 wrote, + 0.5 wd sum ||W||^2, one step on theta_pi
//   5. soft       theta_targ = theta_targ (1 - tau) + theta tau, both nets
//
// State buffer (float32 unless noted), P = Ppi + PQ padded parameters:
//   [0, P) theta   [P, 2P) targets   [2P, 3P) Adam m   [3P, 4P) Adam v   [4P, 5P) gradient scratch (batches > 32 rows)
//   [5P, 5P + 2) int32 step counts: Q, policy
// each plane = [policy | Q]; a net = W0[in][H0p] b0[H0p] W1[in1][H1p] b1[H1p] W2[H1p][out] b2[out], W row-major [in][out];
// H0p / H1p = the hidden widths padded to 32 or 64 (padded units: zero weights in and out, so every gradient, moment
// and decay term of a padded entry is exactly zero; rectify'(0) = 0).  Q's W1 has H0p hidden rows, then A action rows.
//
// The batch is walked in chunks of 32 rows, so the activations take a fixed 57 KB of LDS; the planes theta, targets,
// m, v go into the remaining LDS in that order while they fit whole (dd_plan) and stay in global memory (L2) otherwise.
// A plane is reached through one pointer either way, so residency changes no arithmetic.  Every value has one owner
// thread per phase, phases are separated by __syncthreads(), every sum runs in a fixed order: K updates in one launch
// and K launches of one update give the same bits.
#include <hip/hip_runtime.h>
#include <math.h>
#include "../../include/rllab_amd.h"
#include "capi_util.h"
#include "rl_math.h"

namespace rl {

constexpr int DD_THREADS = 256;
constexpr int DD_CH = 32;                 // batch rows per chunk
constexpr int DD_MAX_D = 32, DD_MAX_A = 8, DD_MAX_H = 64, DD_MAX_B = 128, DD_MAX_K = 16384;
constexpr int DD_DRAWS = 32;              // redraws of a skipped row before the forward walk
constexpr int DD_LDS_LIMIT = 160 * 1024;
constexpr int DD_SGD = 1;
// activation area, in floats
constexpr int DD_X = 0;                                    // [32][D]   observation rows
constexpr int DD_AC = DD_X + DD_CH * DD_MAX_D;             // [32][A]   action rows
constexpr int DD_DA = DD_AC + DD_CH * DD_MAX_A;            // [32][A]   dQ/da, through the output activation
constexpr int DD_BUF = DD_DA + DD_CH * DD_MAX_A;           // six [32][64] hidden buffers
constexpr int DD_NBUF = 6;
constexpr int DD_Y = DD_BUF + DD_NBUF * DD_CH * DD_MAX_H;  // [128] y, q, Q(s, mu(s))
constexpr int DD_Q = DD_Y + DD_MAX_B;
constexpr int DD_QP = DD_Q + DD_MAX_B;
constexpr int DD_DQ = DD_QP + DD_MAX_B;                    // [32] dloss/dq of the chunk
constexpr int DD_TMP = DD_DQ + DD_CH;                      // [32] a scalar head's output
constexpr int DD_AT = DD_TMP + DD_CH;                      // [4]  Adam step sizes a_t: Q, policy
constexpr int DD_ROWS = DD_AT + 4;                         // [128] int32 pool rows of the batch
constexpr int DD_ACT_FLOATS = DD_ROWS + DD_MAX_B;

struct DdOff { int W0, b0, W1, b1, W2, b2, n; };

__host__ __device__ inline DdOff dd_off(int in0, int h0, int in1, int h1, int out) {
    DdOff o;
    o.W0 = 0; o.b0 = in0 * h0; o.W1 = o.b0 + h0; o.b1 = o.W1 + in1 * h1; o.W2 = o.b1 + h1; o.b2 = o.W2 + h1 * out;
    o.n = o.b2 + out;
    return o;
}

static inline int dd_pad(int h) { return h <= 32 ? 32 : 64; }

struct DdK {
    int D, A, H0, H1;                     // H0, H1: padded widths
    int hact, oact, B, K;
    int cap, size, top;
    int qf_method, pi_method;
    float discount, tau, qf_lr, pi_lr, qf_wd, pi_wd;
    uint64_t seed, update_base;
    float* state;
    const float *obs, *act, *rew, *term, *next_obs, *skip;
    const int32_t* indices;
    int32_t* indices_out;
    double* stats;
    float *q_out, *y_out;
    int P, Ppi;
    int lds_plane[4];                     // float offset of theta / targets / m / v in LDS, -1: stays in global memory
};

// planes into LDS behind the activation area, in the order theta, targets, m, v, while they fit whole
static size_t dd_plan(int P, int lds_plane[4]) {
    size_t used = (size_t)DD_ACT_FLOATS * 4;
    for (int k = 0; k < 4; ++k) {
        if (used + (size_t)P * 4 <= (size_t)DD_LDS_LIMIT) {
            lds_plane[k] = (int)(used / 4);
            used += (size_t)P * 4;
        } else {
            lds_plane[k] = -1;
        }
    }
    return used;
}

__device__ __forceinline__ float dd_act(float x, int act) {
    return act == RL_ACT_TANH ? tanhf(x) : (act == RL_ACT_RECTIFY ? fmaxf(x, 0.0f) : x);
}

// derivative from the activation's OUTPUT h
__device__ __forceinline__ float dd_dact(float h, int act) {
    return act == RL_ACT_TANH ? 1.0f - h * h : (act == RL_ACT_RECTIFY ? (h > 0.0f ? 1.0f : 0.0f) : 1.0f);
}

// The layer routines below are __noinline__: each is called from a dozen places of the kernel, one copy keeps it small
// (and clang 22 of ROCm 7.2 crashes in its inliner on the fully inlined kernel).
//
// out[r][j] = act(b[j] + sum_i in_a[r][i] W[i][j] + sum_k in_b[r][k] W[n_a + k][j]),  r < nr, j < nout.
// One owner thread per (r, j), j fastest.  A narrow head (nout < 32) puts several rows on one wavefront: the sum over a
// power-of-two n_a then starts at column r, so the lanes read different LDS banks; the order is fixed per element.
__device__ __noinline__ void dd_dense(const float* W, const float* b, int n_a, const float* in_a, int n_b,
                                      const float* in_b, int nout, int act, float* out, int nr, int tid) {
    const bool rot = (n_a & (n_a - 1)) == 0;
    for (int idx = tid; idx < nr * nout; idx += DD_THREADS) {
        const int r = idx / nout, j = idx - r * nout;
        float acc = b[j];
        const float* x = in_a + r * n_a;
        for (int i = 0; i < n_a; ++i) {
            const int ii = rot ? ((i + r) & (n_a - 1)) : i;
            acc = fmaf(x[ii], W[ii * nout + j], acc);
        }
        for (int k = 0; k < n_b; ++k) acc = fmaf(in_b[r * n_b + k], W[(n_a + k) * nout + j], acc);
        out[r * nout + j] = dd_act(acc, act);
    }
}

// dprev[r][i] = (sum_j d[r][j] W[row0 + i][j]) act'(h[r][i]),  r < nr, i < nprev.  One owner thread per (r, i), i fastest;
// the sum over a power-of-two nout starts at column i (lanes on different banks of W), a fixed order per element.
__device__ __noinline__ void dd_back(const float* W, int row0, int nprev, int nout, const float* d, const float* h,
                                     int act, float* dprev, int nr, int tid) {
    const bool rot = (nout & (nout - 1)) == 0;
    for (int idx = tid; idx < nr * nprev; idx += DD_THREADS) {
        const int r = idx / nprev, i = idx - r * nprev;
        const float* w = W + (row0 + i) * nout;
        const float* dr = d + r * nout;
        float acc = 0.0f;
        for (int j = 0; j < nout; ++j) {
            const int jj = rot ? ((j + i) & (nout - 1)) : j;
            acc = fmaf(dr[jj], w[jj], acc);
        }
        dprev[r * nprev + i] = acc * dd_dact(h[r * nprev + i], act);
    }
}

// What becomes of a parameter's gradient over one chunk: kept in the scratch plane until the batch's last chunk, then
// one step of the net's method.  Entry p is owned by the same thread in every chunk.
struct DdOpt {
    float *th, *m, *v, *gacc;
    int method;
    float lr, a_t, wd;
    bool first, last;
};

__device__ __forceinline__ void dd_sink(const DdOpt& o, int p, float g, bool is_weight) {
    if (!o.first) g = o.gacc[p] + g;
    if (!o.last) {
        o.gacc[p] = g;
        return;
    }
    float w = o.th[p];
    if (is_weight) g = fmaf(o.wd, w, g);
    if (o.method == DD_SGD) {
        w = w - o.lr * g;
    } else {          // lasagne.updates.adam: beta1 0.9, beta2 0.999, epsilon 1e-8
        const float m = 0.9f * o.m[p] + (1.0f - 0.9f) * g;
        const float v = 0.999f * o.v[p] + (1.0f - 0.999f) * (g * g);
        o.m[p] = m;
        o.v[p] = v;
        w = w - o.a_t * m / (sqrtf(v) + 1e-8f);
    }
    o.th[p] = w;
}

// gradient of one dense layer over the chunk: W[i][j] += sum_r in[r][i] d[r][j], b[j] += sum_r d[r][j]; the layer's
// W and b are adjacent in the net (offset off), inputs as dd_dense takes them
__device__ __noinline__ void dd_layer_grad(const DdOpt& o, int off, int n_a, const float* in_a, int n_b, const float* in_b,
                                           int nout, const float* d, int nr, int tid) {
    const int nW = (n_a + n_b) * nout;
    for (int e = tid; e < nW + nout; e += DD_THREADS) {
        float g = 0.0f;
        if (e < nW) {
            const int i = e / nout, j = e - i * nout;
            const float* src = i < n_a ? in_a + i : in_b + (i - n_a);
            const int stride = i < n_a ? n_a : n_b;
            for (int r = 0; r < nr; ++r) g = fmaf(src[r * stride], d[r * nout + j], g);
        } else {
            const int j = e - nW;
            for (int r = 0; r < nr; ++r) g += d[r * nout + j];
        }
        dd_sink(o, off + e, g, e < nW);
    }
}

// Pool row of slot b of update counter c: Philox4x32-10 word 0 at counters (attempt, b, c_lo, c_hi), key = seed;
// logical index = (word * size) >> 32, physical row = (top - size + index) mod cap; a row with skip = 1 is redrawn with
// the next attempt, after DD_DRAWS attempts the walk goes forward (mod size) to the first kept row.  At most
// DD_DRAWS + size reads: it ends for any pool (an all-skip pool gives the last drawn row).
__device__ __noinline__ int dd_draw_row(const DdK& a, uint32_t b, uint64_t c) {
    const uint32_t size = (uint32_t)a.size, cap = (uint32_t)a.cap;
    const uint32_t base = (uint32_t)a.top + cap - size;
    uint32_t index = 0;
    for (uint32_t attempt = 0; attempt < (uint32_t)DD_DRAWS; ++attempt) {
        const Philox4 p = philox4x32_10(attempt, b, (uint32_t)c, (uint32_t)(c >> 32), (uint32_t)a.seed,
                                        (uint32_t)(a.seed >> 32));
        index = (uint32_t)(((uint64_t)p.v[0] * size) >> 32);
        const uint32_t row = (base + index) % cap;
        if (a.skip[row] == 0.0f) return (int)row;
    }
    for (uint32_t w = 1; w <= size; ++w) {
        const uint32_t row = (base + (index + w) % size) % cap;
        if (a.skip[row] == 0.0f) return (int)row;
    }
    return (int)((base + index) % cap);
}

// b^t by squaring: a function of t alone, so the step size of update t is the same in any split into launches
__device__ __forceinline__ double dd_powi(double b, int t) {
    double r = 1.0;
    for (; t > 0; t >>= 1) {
        if (t & 1) r *= b;
        b *= b;
    }
    return r;
}

__device__ __forceinline__ double dd_wave_sum(double x) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) x += __shfl_xor(x, s, 64);
    return x;
}

__device__ __forceinline__ void dd_gather(float* dst, const float* src, const int* rows, int nr, int width, int tid) {
    for (int idx = tid; idx < nr * width; idx += DD_THREADS) {
        const int r = idx / width, i = idx - r * width;
        dst[idx] = src[(size_t)rows[r] * width + i];
    }
}

__global__ void __launch_bounds__(DD_THREADS) ddpg_update_kernel(DdK a) {
    extern __shared__ float lds[];
    const int tid = threadIdx.x;
    const int D = a.D, A = a.A, H0 = a.H0, H1 = a.H1, B = a.B, P = a.P;
    const DdOff op = dd_off(D, H0, H0, H1, A), oq = dd_off(D, H0, H0 + A, H1, 1);
    float* plane[4];
    for (int k = 0; k < 4; ++k) {
        plane[k] = a.lds_plane[k] >= 0 ? lds + a.lds_plane[k] : a.state + (size_t)k * P;
        if (a.lds_plane[k] >= 0)
            for (int i = tid; i < P; i += DD_THREADS) plane[k][i] = a.state[(size_t)k * P + i];
    }
    float* gacc = a.state + (size_t)4 * P;
    int32_t* counts = reinterpret_cast<int32_t*>(a.state + (size_t)5 * P);
    int t_q = counts[0], t_pi = counts[1];
    float *th_pi = plane[0], *th_q = plane[0] + a.Ppi;
    const float *tg_pi = plane[1], *tg_q = plane[1] + a.Ppi;

    float *X = lds + DD_X, *AC = lds + DD_AC, *DA = lds + DD_DA;
    float *Hq0 = lds + DD_BUF, *Hq1 = Hq0 + DD_CH * DD_MAX_H, *G0 = Hq1 + DD_CH * DD_MAX_H, *G1 = G0 + DD_CH * DD_MAX_H,
          *Hp0 = G1 + DD_CH * DD_MAX_H, *Hp1 = Hp0 + DD_CH * DD_MAX_H;
    float *s_y = lds + DD_Y, *s_q = lds + DD_Q, *s_qp = lds + DD_QP, *s_dq = lds + DD_DQ, *s_tmp = lds + DD_TMP,
          *s_at = lds + DD_AT;
    int* s_rows = reinterpret_cast<int*>(lds + DD_ROWS);
    const int nchunk = (B + DD_CH - 1) / DD_CH;
    const float inv_b = 1.0f / (float)B;
    double acc_stats[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) acc_stats[k] = 0.0;
    __syncthreads();

    for (int u = 0; u < a.K; ++u) {
        // ---- 1. the batch's pool rows, and this update's Adam step sizes --------------------------------------------
        if (tid < B) {
            int row;
            if (a.indices) row = min(max(a.indices[(size_t)u * B + tid], 0), a.cap - 1);
            else row = dd_draw_row(a, (uint32_t)tid, a.update_base + (uint64_t)u);
            s_rows[tid] = row;
            if (a.indices_out) a.indices_out[(size_t)u * B + tid] = row;
        }
        t_q += 1;
        t_pi += 1;
        if (tid == 64 || tid == 128) {    // a_t = lr sqrt(1 - beta2^t) / (1 - beta1^t), float64 like the host would form it
            const bool q = tid == 64;
            const int t = q ? t_q : t_pi;
            const double lr = (double)(q ? a.qf_lr : a.pi_lr);
            s_at[q ? 0 : 1] = (float)(lr * sqrt(1.0 - dd_powi(0.999, t)) / (1.0 - dd_powi(0.9, t)));
        }
        __syncthreads();

        // ---- 2 + 3. targets and the Q step, chunk by chunk ----------------------------------------------------------
        DdOpt oQ;
        oQ.th = th_q; oQ.m = plane[2] + a.Ppi; oQ.v = plane[3] + a.Ppi; oQ.gacc = gacc + a.Ppi;
        oQ.method = a.qf_method; oQ.lr = a.qf_lr; oQ.a_t = s_at[0]; oQ.wd = a.qf_wd;
        for (int c = 0; c < nchunk; ++c) {
            const int r0 = c * DD_CH, nr = min(DD_CH, B - r0);
            const int* rows = s_rows + r0;
            dd_gather(X, a.next_obs, rows, nr, D, tid);
            __syncthreads();
            dd_dense(tg_pi + op.W0, tg_pi + op.b0, D, X, 0, nullptr, H0, a.hact, Hq0, nr, tid);
            __syncthreads();
            dd_dense(tg_pi + op.W1, tg_pi + op.b1, H0, Hq0, 0, nullptr, H1, a.hact, Hq1, nr, tid);
            __syncthreads();
            dd_dense(tg_pi + op.W2, tg_pi + op.b2, H1, Hq1, 0, nullptr, A, a.oact, AC, nr, tid);
            __syncthreads();
            dd_dense(tg_q + oq.W0, tg_q + oq.b0, D, X, 0, nullptr, H0, a.hact, Hq0, nr, tid);
            __syncthreads();
            dd_dense(tg_q + oq.W1, tg_q + oq.b1, H0, Hq0, A, AC, H1, a.hact, Hq1, nr, tid);
            __syncthreads();
            dd_dense(tg_q + oq.W2, tg_q + oq.b2, H1, Hq1, 0, nullptr, 1, RL_ACT_IDENTITY, s_tmp, nr, tid);
            __syncthreads();
            if (tid < nr) {
                const int row = rows[tid];
                s_y[r0 + tid] = a.rew[row] + (1.0f - a.term[row]) * a.discount * s_tmp[tid];
            }
            dd_gather(X, a.obs, rows, nr, D, tid);
            dd_gather(AC, a.act, rows, nr, A, tid);
            __syncthreads();
            dd_dense(th_q + oq.W0, th_q + oq.b0, D, X, 0, nullptr, H0, a.hact, Hq0, nr, tid);
            __syncthreads();
            dd_dense(th_q + oq.W1, th_q + oq.b1, H0, Hq0, A, AC, H1, a.hact, Hq1, nr, tid);
            __syncthreads();
            dd_dense(th_q + oq.W2, th_q + oq.b2, H1, Hq1, 0, nullptr, 1, RL_ACT_IDENTITY, s_tmp, nr, tid);
            __syncthreads();
            if (tid < nr) {
                const float q = s_tmp[tid];
                s_q[r0 + tid] = q;
                s_dq[tid] = 2.0f * (q - s_y[r0 + tid]) * inv_b;      // d mean((y - q)^2) / dq
            }
            __syncthreads();
            dd_back(th_q + oq.W2, 0, H1, 1, s_dq, Hq1, a.hact, G1, nr, tid);
            __syncthreads();
            dd_back(th_q + oq.W1, 0, H0, H1, G1, Hq0, a.hact, G0, nr, tid);
            __syncthreads();
            oQ.first = c == 0;
            oQ.last = c == nchunk - 1;
            dd_layer_grad(oQ, oq.W0, D, X, 0, nullptr, H0, G0, nr, tid);
            dd_layer_grad(oQ, oq.W1, H0, Hq0, A, AC, H1, G1, nr, tid);
            dd_layer_grad(oQ, oq.W2, H1, Hq1, 0, nullptr, 1, s_dq, nr, tid);
            __syncthreads();
        }
        if (tid < B) {
            if (a.q_out) a.q_out[(size_t)u * B + tid] = s_q[tid];
            if (a.y_out) a.y_out[(size_t)u * B + tid] = s_y[tid];
        }

        // ---- 4. the policy step at the Q parameters just written ----------------------------------------------------
        DdOpt oP;
        oP.th = th_pi; oP.m = plane[2]; oP.v = plane[3]; oP.gacc = gacc;
        oP.method = a.pi_method; oP.lr = a.pi_lr; oP.a_t = s_at[1]; oP.wd = a.pi_wd;
        for (int c = 0; c < nchunk; ++c) {
            const int r0 = c * DD_CH, nr = min(DD_CH, B - r0);
            const int* rows = s_rows + r0;
            dd_gather(X, a.obs, rows, nr, D, tid);
            __syncthreads();
            dd_dense(th_pi + op.W0, th_pi + op.b0, D, X, 0, nullptr, H0, a.hact, Hp0, nr, tid);
            __syncthreads();
            dd_dense(th_pi + op.W1, th_pi + op.b1, H0, Hp0, 0, nullptr, H1, a.hact, Hp1, nr, tid);
            __syncthreads();
            dd_dense(th_pi + op.W2, th_pi + op.b2, H1, Hp1, 0, nullptr, A, a.oact, AC, nr, tid);
            __syncthreads();
            dd_dense(th_q + oq.W0, th_q + oq.b0, D, X, 0, nullptr, H0, a.hact, Hq0, nr, tid);
            __syncthreads();
            dd_dense(th_q + oq.W1, th_q + oq.b1, H0, Hq0, A, AC, H1, a.hact, Hq1, nr, tid);
            __syncthreads();
            dd_dense(th_q + oq.W2, th_q + oq.b2, H1, Hq1, 0, nullptr, 1, RL_ACT_IDENTITY, s_tmp, nr, tid);
            if (tid < nr) s_dq[tid] = -inv_b;                         // d(-mean Q) / dQ
            __syncthreads();
            if (tid < nr) s_qp[r0 + tid] = s_tmp[tid];
            dd_back(th_q + oq.W2, 0, H1, 1, s_dq, Hq1, a.hact, G1, nr, tid);
            __syncthreads();
            dd_back(th_q + oq.W1, H0, A, H1, G1, AC, a.oact, DA, nr, tid);          // the action rows of Q's W1
            __syncthreads();
            dd_back(th_pi + op.W2, 0, H1, A, DA, Hp1, a.hact, G0, nr, tid);          // G0: the policy's layer-1 deltas
            __syncthreads();
            dd_back(th_pi + op.W1, 0, H0, H1, G0, Hp0, a.hact, Hq0, nr, tid);        // Hq0: the policy's layer-0 deltas
            __syncthreads();
            oP.first = c == 0;
            oP.last = c == nchunk - 1;
            dd_layer_grad(oP, op.W0, D, X, 0, nullptr, H0, Hq0, nr, tid);
            dd_layer_grad(oP, op.W1, H0, Hp0, 0, nullptr, H1, G0, nr, tid);
            dd_layer_grad(oP, op.W2, H1, Hp1, 0, nullptr, A, DA, nr, tid);
            __syncthreads();
        }

        // ---- 5. soft targets from the parameters just written; the update's statistics on wavefront 0 ---------------
        {
            float* tg = plane[1];
            const float* th = plane[0];
            const float keep = 1.0f - a.tau;
            for (int i = tid; i < P; i += DD_THREADS) tg[i] = tg[i] * keep + th[i] * a.tau;
        }
        if (tid < 64) {
            double sq = 0, saq = 0, sy = 0, say = 0, sd = 0, sl = 0, sp = 0;
            for (int b = tid; b < B; b += 64) {
                const double q = (double)s_q[b], y = (double)s_y[b];
                sq += q; saq += fabs(q); sy += y; say += fabs(y); sd += fabs(q - y); sl += (y - q) * (y - q);
                sp += (double)s_qp[b];
            }
            acc_stats[0] += dd_wave_sum(sl) / (double)B;
            acc_stats[1] += -dd_wave_sum(sp) / (double)B;
            acc_stats[2] += 1.0;
            acc_stats[3] += dd_wave_sum(sq);
            acc_stats[4] += dd_wave_sum(saq);
            acc_stats[5] += dd_wave_sum(sy);
            acc_stats[6] += dd_wave_sum(say);
            acc_stats[7] += dd_wave_sum(sd);
            acc_stats[8] += (double)B;
        }
        __syncthreads();
    }

    for (int k = 0; k < 4; ++k)
        if (a.lds_plane[k] >= 0)
            for (int i = tid; i < P; i += DD_THREADS) a.state[(size_t)k * P + i] = plane[k][i];
    if (tid == 0) {
        counts[0] = t_q;
        counts[1] = t_pi;
        if (a.stats)
            for (int k = 0; k < 9; ++k) a.stats[k] += acc_stats[k];
    }
}

static int dd_net_floats(int D, int A, int H0p, int H1p, int* Ppi) {
    const DdOff op = dd_off(D, H0p, H0p, H1p, A), oq = dd_off(D, H0p, H0p + A, H1p, 1);
    if (Ppi) *Ppi = op.n;
    return op.n + oq.n;
}

static bool dd_shape_ok(int D, int A, int H0, int H1) {
    return D >= 1 && D <= DD_MAX_D && A >= 1 && A <= DD_MAX_A && H0 >= 1 && H0 <= DD_MAX_H && H1 >= 1 && H1 <= DD_MAX_H;
}

}  // namespace rl

using namespace rl;

extern "C" size_t rl_ddpg_state_bytes(int obs_dim, int act_dim, int hidden0, int hidden1) {
    if (!dd_shape_ok(obs_dim, act_dim, hidden0, hidden1)) return 0;
    const size_t P = (size_t)dd_net_floats(obs_dim, act_dim, dd_pad(hidden0), dd_pad(hidden1), nullptr);
    return ((5 * P + 2) * 4 + 15) / 16 * 16;
}

extern "C" int rl_ddpg_update(const rl_ddpg_args* g, void* stream) {
    if (!g) return set_error(RL_ERR_ARG, "rl_ddpg_update: NULL arguments");
    if (g->obs_dim < 1 || g->act_dim < 1 || g->hidden0 < 1 || g->hidden1 < 1)
        return set_error(RL_ERR_ARG, "rl_ddpg_update: obs_dim, act_dim, hidden0, hidden1 must be positive");
    if (!dd_shape_ok(g->obs_dim, g->act_dim, g->hidden0, g->hidden1))
        return set_error(RL_ERR_UNSUPPORTED, "rl_ddpg_update: obs_dim %d, act_dim %d, hidden (%d, %d): the kernel runs "
                         "obs_dim <= %d, act_dim <= %d and two hidden layers of at most %d units", g->obs_dim, g->act_dim,
                         g->hidden0, g->hidden1, DD_MAX_D, DD_MAX_A, DD_MAX_H);
    if (g->hidden_activation != RL_ACT_TANH && g->hidden_activation != RL_ACT_RECTIFY)
        return set_error(RL_ERR_UNSUPPORTED, "rl_ddpg_update: hidden_activation %d (RL_ACT_TANH or RL_ACT_RECTIFY)",
                         g->hidden_activation);
    if (g->output_activation != RL_ACT_TANH && g->output_activation != RL_ACT_IDENTITY)
        return set_error(RL_ERR_UNSUPPORTED, "rl_ddpg_update: output_activation %d (RL_ACT_TANH or RL_ACT_IDENTITY)",
                         g->output_activation);
    if (g->batch < 1 || g->batch > DD_MAX_B)
        return set_error(RL_ERR_UNSUPPORTED, "rl_ddpg_update: batch %d (1 .. %d)", g->batch, DD_MAX_B);
    if (g->n_updates < 1 || g->n_updates > DD_MAX_K)
        return set_error(RL_ERR_UNSUPPORTED, "rl_ddpg_update: n_updates %d (1 .. %d per launch)", g->n_updates, DD_MAX_K);
    if (g->capacity < 1 || g->size < 1 || g->size > g->capacity || g->top < 0 || g->top >= g->capacity)
        return set_error(RL_ERR_ARG, "rl_ddpg_update: pool capacity %d, size %d, top %d (1 <= size <= capacity, "
                         "0 <= top < capacity)", g->capacity, g->size, g->top);
    if (g->size <= g->batch)
        return set_error(RL_ERR_ARG, "rl_ddpg_update: pool size %d must exceed the batch %d", g->size, g->batch);
    if ((g->qf_method != 0 && g->qf_method != DD_SGD) || (g->policy_method != 0 && g->policy_method != DD_SGD))
        return set_error(RL_ERR_ARG, "rl_ddpg_update: update method %d / %d (0 adam, 1 sgd)", g->qf_method, g->policy_method);
    const float fl[6] = {g->discount, g->tau, g->qf_learning_rate, g->policy_learning_rate, g->qf_weight_decay,
                         g->policy_weight_decay};
    for (int k = 0; k < 6; ++k)
        if (!isfinite(fl[k])) return set_error(RL_ERR_ARG, "rl_ddpg_update: a non-finite rate, decay, discount or tau");
    if (g->tau < 0.0f || g->tau > 1.0f) return set_error(RL_ERR_ARG, "rl_ddpg_update: tau %g (0 .. 1)", (double)g->tau);
    if (!g->state || !g->obs || !g->act || !g->rew || !g->term || !g->next_obs || !g->skip)
        return set_error(RL_ERR_ARG, "rl_ddpg_update: NULL state or pool plane");

    DdK a;
    a.D = g->obs_dim; a.A = g->act_dim; a.H0 = dd_pad(g->hidden0); a.H1 = dd_pad(g->hidden1);
    a.hact = g->hidden_activation; a.oact = g->output_activation; a.B = g->batch; a.K = g->n_updates;
    a.cap = g->capacity; a.size = g->size; a.top = g->top;
    a.qf_method = g->qf_method; a.pi_method = g->policy_method;
    a.discount = g->discount; a.tau = g->tau; a.qf_lr = g->qf_learning_rate; a.pi_lr = g->policy_learning_rate;
    a.qf_wd = g->qf_weight_decay; a.pi_wd = g->policy_weight_decay;
    a.seed = g->seed; a.update_base = g->update_base;
    a.state = (float*)g->state;
    a.obs = (const float*)g->obs; a.act = (const float*)g->act; a.rew = (const float*)g->rew;
    a.term = (const float*)g->term; a.next_obs = (const float*)g->next_obs; a.skip = (const float*)g->skip;
    a.indices = (const int32_t*)g->indices; a.indices_out = (int32_t*)g->indices_out;
    a.stats = (double*)g->stats; a.q_out = (float*)g->q_out; a.y_out = (float*)g->y_out;
    a.P = dd_net_floats(a.D, a.A, a.H0, a.H1, &a.Ppi);
    const size_t lds = dd_plan(a.P, a.lds_plane);
    static bool attr_set = false;
    if (!attr_set) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(ddpg_update_kernel),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, DD_LDS_LIMIT);
        if (e != hipSuccess) return set_error(RL_ERR_HIP, "hipFuncSetAttribute: %s", hipGetErrorString(e));
        attr_set = true;
    }
    hipLaunchKernelGGL(ddpg_update_kernel, dim3(1), dim3(DD_THREADS), lds, (hipStream_t)stream, a);
    return check_launch("ddpg_update_kernel");
}
