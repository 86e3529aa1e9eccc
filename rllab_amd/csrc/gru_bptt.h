// gru_bptt.h -- what the update kernels of the two GRU policies (gru_bptt_kernels.hip: GaussianGRUPolicy,
// categorical_gru_bptt_kernels.hip: CategoricalGRUPolicy) share next to the GRU step of gru_cell.h: the gate sums of one
// block of units on their own, one step of the tangent sweep, the backward sweep, the weight sums on the matrix cores, the
// fixed-order finish and the workspace plan.
//
// gru_cell evaluates a whole step and keeps the gates to itself; the backward sweep and the tangent sweep need r, u, c
// and h W_hc of the step they are at.  gru_preact4 / gru_hidden4 RESTATE the sums of gru_cell -- bias, then the inputs,
// then the hidden units, each in index order, one float32 FMA per term -- so a gate recomputed here from the h the
// forward sweep stored is the gate the forward sweep used, bit for bit.  gru_cell itself is left as it is: three rollout
// kernels are pinned to its instruction stream.
//
// The shared kernels are templates over two things a policy family brings:
//   Dev   the batch as its sweeps see it (BpttDev here, CatBpttDev in categorical_gru_bptt_kernels.hip).  Read by name:
//         n, T, include_action, B, inv_count, theta, v, start, part, hs, dr, du, dc, rdc, dmean, wpart.
//   In    the input of one step of one lane (DensePlanes: x = [obs, prev_action] from float planes; OneHotPlanes: two
//         row indices from int planes): input_dim(a), load(a, s, first), input() -- what gru_preact4 adds x W_x* with --
//         and N_LS, the rows of the family's own that follow GruLayout's `total` (the Gaussian log-std).
//   Rows  [x; 1] of a sample as the left operand of the weight sums (DenseRows, OneHotRows): x(a, row, s, start) with DI.
#pragma once
#include <stdint.h>
#include "gru_cell.h"

namespace rl {

// sum_k h[k] W_h*[k][j .. j + 3] added to the three sums, k in index order (the hidden-unit loop of gru_cell)
template <int H, int NOUT, class W>
__device__ __forceinline__ void gru_hidden4(const W& w, const GruLayout<H, NOUT>& off, int DI, const float* hc, int j,
                                            F4& ar, F4& au, F4& ah) {
    const int hr = off.wh(0, DI) + j, hu = off.wh(1, DI) + j, hcw = off.wh(2, DI) + j;
#pragma unroll 8
    for (int k = 0; k < H; ++k) {
        const float h = hc[k * WV];
        const F4 wr = w.load4(hr + k * H), wu = w.load4(hu + k * H), wc = w.load4(hcw + k * H);
#pragma unroll
        for (int u = 0; u < GRU_UB; ++u) {
            ar.v[u] = __builtin_fmaf(h, wr.v[u], ar.v[u]);
            au.v[u] = __builtin_fmaf(h, wu.v[u], au.v[u]);
            ah.v[u] = __builtin_fmaf(h, wc.v[u], ah.v[u]);
        }
    }
}

// the sums of units j .. j + 3 ahead of the nonlinearities: ar, au (r = sigmoid(ar), u = sigmoid(au)), ax = x W_xc + b_c
// and ah = h W_hc (c = tanh(ax + r ah)).  With `w` the tangent vector instead of the parameters: the part of the sums'
// tangents that comes from the weights moving.
template <int H, int NOUT, class W, class Input>
__device__ __forceinline__ void gru_preact4(const W& w, const GruLayout<H, NOUT>& off, int DI, const Input& input,
                                            const float* hc, int j, F4& ar, F4& au, F4& ax, F4& ah) {
    ar = w.load4(off.b(0, DI) + j); au = w.load4(off.b(1, DI) + j); ax = w.load4(off.b(2, DI) + j);
    ah = F4{{0.0f, 0.0f, 0.0f, 0.0f}};
    input(w, off.wx(0), off.wx(1), off.wx(2), j, ar, au, ax);
    gru_hidden4(w, off, DI, hc, j, ar, au, ah);
}

constexpr int BPTT_PART = 20;     // doubles per workgroup of a sweep: loss, KL, sum w, d log_std [<= 8], d b_out [<= 8]
constexpr int BPTT_MAX_CHUNKS = 256;

// A recurrent Gaussian batch on its dense planes (sample s = t * n + i of env column i) and the workspace of its update
// passes.
struct BpttDev {
    int n, T, include_action;
    size_t B;                   // T * n
    double inv_count;
    const float *theta, *v, *obs, *actions, *adv, *old_means, *old_log_std, *weights;
    const uint8_t* start;
    float* means;               // NULL, or where the forward sweep leaves its means [DA][B]
    double* part;               // [workgroups of a sweep][BPTT_PART]
    float *hs;                  // [H][B]  h' of every step (the forward sweep of the gradient pass)
    float *dr, *du, *dc, *rdc;  // [H][B]  the backward sweep's cotangents of the gate sums; rdc = r * dc
    float* dmean;               // [NOUT][B] cotangent of the outputs (the means; the logits)
    float* wpart;               // [chunks][P4] the weight gradient's partial sums
};

// sigma of a log-std row entry, in float64 from the float32 value (new and old the same expression: their difference
// vanishes identically at equal inputs)
__device__ __forceinline__ double sigma_of(float log_std) { return exp((double)log_std); }

// x = [obs, prev_action] of a lane's step from the float planes obs [DO][B] and actions [DA][B]
template <int DO, int DA, int H>
struct DensePlanes {
    static constexpr int N_LS = DA;
    float o[DO], pa[DA];
    bool include_action;
    template <class Dev>
    static __device__ __forceinline__ int input_dim(const Dev& a) { return DO + (a.include_action ? DA : 0); }
    template <class Dev>
    __device__ __forceinline__ void load(const Dev& a, size_t s, bool first) {
        include_action = a.include_action != 0;
#pragma unroll
        for (int k = 0; k < DA; ++k) pa[k] = first ? 0.0f : a.actions[(size_t)k * a.B + s - a.n];
#pragma unroll
        for (int d = 0; d < DO; ++d) o[d] = a.obs[(size_t)d * a.B + s];
    }
    __device__ __forceinline__ DenseInput<DO, DA, H> input() const { return DenseInput<DO, DA, H>{o, pa, include_action}; }
};

// row `row` of [x; 1] at sample s (st: the step starts a path) for the weight sums
struct DenseRows {
    int DO, DI;
    template <class Dev>
    __device__ __forceinline__ float operator()(const Dev& a, int row, size_t s, bool st) const {
        if (row < DO) return a.obs[(size_t)row * a.B + s];
        if (row < DI) return st ? 0.0f : a.actions[(size_t)(row - DO) * a.B + s - (size_t)a.n];
        return row == DI ? 1.0f : 0.0f;
    }
};

template <int NOUT, class Dev>
__device__ __forceinline__ void write_partials(const Dev& a, double loss, double kl, double sw, const double* dls,
                                               const double* dbo) {
    double* p = a.part + (size_t)blockIdx.x * BPTT_PART;
    loss = wave_sum(loss); kl = wave_sum(kl); sw = wave_sum(sw);
    if (threadIdx.x == 0) { p[0] = loss; p[1] = kl; p[2] = sw; }
#pragma unroll
    for (int k = 0; k < NOUT; ++k) {
        const double l = wave_sum(dls[k]), b = wave_sum(dbo[k]);
        if (threadIdx.x == 0) { p[3 + k] = l; p[3 + 8 + k] = b; }
    }
}

// One step of the tangent sweep of one lane: from h_prev (column hp), the tangent of h_prev (column dhc) and the step's
// input, the tangent of h' into column dhn and the tangent of the outputs added to tm (the caller starts it at v's b_out).
// LOGITS: also the outputs themselves added to out (started at theta's b_out) -- gru_cell's FMAs in gru_cell's order.
template <int H, int NOUT, bool LOGITS, class Input>
__device__ __forceinline__ void gru_tangent_step(const LdsWeights& th, const LdsWeights& vw, const GruLayout<H, NOUT>& off,
                                                 int DI, const Input& in, const float* hp, const float* dhc, float* dhn,
                                                 float* tm, float* out) {
#pragma unroll 1
    for (int j = 0; j < H; j += GRU_UB) {
        F4 ar, au, ax, ah, tr, tu, tx, tah;
        gru_preact4(th, off, DI, in, hp, j, ar, au, ax, ah);
        gru_preact4(vw, off, DI, in, hp, j, tr, tu, tx, tah);       // the weights move ...
        gru_hidden4(th, off, DI, dhc, j, tr, tu, tah);              // ... and so does h
#pragma unroll
        for (int u = 0; u < GRU_UB; ++u) {
            const float r = fsigmoid(ar.v[u]), g = fsigmoid(au.v[u]);
            const float c = ftanh(__builtin_fmaf(r, ah.v[u], ax.v[u]));
            const float h_old = hp[(j + u) * WV];
            const float h_new = __builtin_fmaf(g, c, (1.0f - g) * h_old);
            const float dr = r * (1.0f - r) * tr.v[u], dg = g * (1.0f - g) * tu.v[u];
            const float dc = (1.0f - c * c) * (tx.v[u] + dr * ah.v[u] + r * tah.v[u]);
            const float dh = dg * (c - h_old) + g * dc + (1.0f - g) * dhc[(j + u) * WV];
            dhn[(j + u) * WV] = dh;
#pragma unroll
            for (int k = 0; k < NOUT; ++k) {
                const float wo = th.load(off.w_out + (j + u) * NOUT + k);
                if (LOGITS) out[k] = __builtin_fmaf(h_new, wo, out[k]);
                tm[k] = __builtin_fmaf(dh, wo, tm[k]);
                tm[k] = __builtin_fmaf(h_new, vw.load(off.w_out + (j + u) * NOUT + k), tm[k]);
            }
        }
    }
}

// The backward sweep, t = T - 1 .. 0: carries dh per lane, recomputes the gates of the step from the stored h, leaves the
// cotangents of the three gate sums of every sample in the workspace.
// LDS: theta [P4], the tiles of dr, du and r * dc of the step, then h_prev and dh (GruLanes' hc / hn).
template <class In, int NOUT, int H, class Dev>
__global__ void __launch_bounds__(GRU_BLOCK) gru_bwd_kernel(Dev a, int w_floats) {
    const int DI = In::input_dim(a);
    const GruLayout<H, NOUT> off(DI);
    const int n_theta = off.total + In::N_LS, P4 = (n_theta + 3) & ~3;
    GruLanes<H> lanes(a.theta, n_theta, w_floats);
    const int i = blockIdx.x * GRU_BLOCK + threadIdx.x;
    if (i >= a.n) return;                     // no cross-lane traffic from here on
    const LdsWeights th{lanes.w};
    float* smem = const_cast<float*>(lanes.w);
    float* tr = smem + P4 + threadIdx.x;
    float* tu = tr + H * WV;
    float* tc = tu + H * WV;
    float* hp = lanes.hc;
    float* dh = lanes.hn;
    const size_t B = a.B;
    const int hr = off.wh(0, DI), hu = off.wh(1, DI), hcw = off.wh(2, DI);
#pragma unroll 1
    for (int t = a.T - 1; t >= 0; --t) {
        const size_t s = (size_t)t * a.n + i;
        // nothing comes back from a step that started from h0
        if (t == a.T - 1 || a.start[s + a.n]) {
#pragma unroll 1
            for (int k = 0; k < H; ++k) dh[k * WV] = 0.0f;
        }
        const bool first = t == 0 || a.start[s];
        if (first) {
#pragma unroll 1
            for (int k = 0; k < H; ++k) hp[k * WV] = th.load(k);
        } else {
#pragma unroll 4
            for (int k = 0; k < H; ++k) hp[k * WV] = a.hs[(size_t)k * B + s - a.n];
        }
        In step;
        step.load(a, s, first);
        float dm[NOUT];
#pragma unroll
        for (int k = 0; k < NOUT; ++k) dm[k] = a.dmean[(size_t)k * B + s];
        const auto in = step.input();
        // the gates of the step and the cotangents of their sums; dh becomes its direct part (1 - u) dh
#pragma unroll 1
        for (int j = 0; j < H; j += GRU_UB) {
            F4 ar, au, ax, ah;
            gru_preact4(th, off, DI, in, hp, j, ar, au, ax, ah);
#pragma unroll
            for (int u = 0; u < GRU_UB; ++u) {
                const float r = fsigmoid(ar.v[u]), g = fsigmoid(au.v[u]);
                const float c = ftanh(__builtin_fmaf(r, ah.v[u], ax.v[u]));
                float d = dh[(j + u) * WV];
#pragma unroll
                for (int k = 0; k < NOUT; ++k) d = __builtin_fmaf(dm[k], th.load(off.w_out + (j + u) * NOUT + k), d);
                const float dc = d * g * (1.0f - c * c);
                const float du = d * (c - hp[(j + u) * WV]) * g * (1.0f - g);
                const float dr = dc * ah.v[u] * r * (1.0f - r);
                const float rdc = r * dc;
                dh[(j + u) * WV] = (1.0f - g) * d;
                tr[(j + u) * WV] = dr; tu[(j + u) * WV] = du; tc[(j + u) * WV] = rdc;
                const size_t e = (size_t)(j + u) * B + s;
                a.dr[e] = dr; a.du[e] = du; a.dc[e] = dc; a.rdc[e] = rdc;
            }
        }
        // dh_prev[k] = (1 - u[k]) dh[k] + sum_j W_hr[k][j] dr[j] + W_hu[k][j] du[j] + W_hc[k][j] r[j] dc[j]: the forward
        // pass's 16-byte broadcast reads with the roles of the two indices swapped
#pragma unroll 1
        for (int k = 0; k < H; k += GRU_UB) {
            float acc[GRU_UB];
#pragma unroll
            for (int q = 0; q < GRU_UB; ++q) acc[q] = dh[(k + q) * WV];
#pragma unroll 2
            for (int j = 0; j < H; j += GRU_UB) {
                float vr[GRU_UB], vu[GRU_UB], vc[GRU_UB];
#pragma unroll
                for (int u = 0; u < GRU_UB; ++u) { vr[u] = tr[(j + u) * WV]; vu[u] = tu[(j + u) * WV]; vc[u] = tc[(j + u) * WV]; }
#pragma unroll
                for (int q = 0; q < GRU_UB; ++q) {
                    const F4 wr = th.load4(hr + (k + q) * H + j), wu = th.load4(hu + (k + q) * H + j),
                             wc = th.load4(hcw + (k + q) * H + j);
#pragma unroll
                    for (int u = 0; u < GRU_UB; ++u) {
                        acc[q] = __builtin_fmaf(wr.v[u], vr[u], acc[q]);
                        acc[q] = __builtin_fmaf(wu.v[u], vu[u], acc[q]);
                        acc[q] = __builtin_fmaf(wc.v[u], vc[u], acc[q]);
                    }
                }
            }
#pragma unroll
            for (int q = 0; q < GRU_UB; ++q) dh[(k + q) * WV] = acc[q];
        }
    }
}

// 32-row blocks of [x; 1]: DI + 1 rows
__host__ __device__ inline int bptt_input_blocks(int DI) { return (DI + 1 + 31) / 32; }

// One wavefront: the sums over the samples [c L, (c + 1) L) of one 32-row block of [x; 1] or of h_prev against one
// 32-column block of dr, du, dc (r dc for h_prev) -- three 32 x 32 tiles -- or of 32 units of h' against the cotangent of
// the outputs.  blockIdx.y: bptt_input_blocks(DI) row blocks of [x; 1], then H / 32 of h_prev, each x H / 32 column blocks;
// then H / 32 unit blocks of W_out.
// MFMA operands (v_mfma_f32_32x32x2_f32): lane l holds row l & 31 of the left factor and column l & 31 of the right one
// at sample s0 + (l >> 5); the result's column is l & 31, its rows frag_unit(register, l >> 5).
template <int H, class Rows, class Dev>
__global__ void __launch_bounds__(WV) gru_wgrad_kernel(Dev a, Rows x, int NOUT, int P4, int L) {
    constexpr int NB = H / 32;
    const int DI = x.DI, NXB = bptt_input_blocks(DI);
    const GruLayout<H, 1> off(DI);            // (the offsets used here do not depend on the number of outputs)
    const int l = threadIdx.x, i = l & 31, half = l >> 5, job = blockIdx.y;
    const size_t B = a.B, n = (size_t)a.n;
    const size_t s_begin = (size_t)blockIdx.x * L, s_end = s_begin + L < B ? s_begin + L : B;
    float* out = a.wpart + (size_t)blockIdx.x * P4;
    if (job < (NXB + NB) * NB) {
        const int ta = job / NB, jb = job % NB;
        const size_t col = (size_t)(32 * jb + i) * B;
        const float* br = a.dr + col;
        const float* bu = a.du + col;
        const float* bc = (ta < NXB ? a.dc : a.rdc) + col;
        f32x16 cr = {0}, cu = {0}, cc = {0};
        for (size_t s0 = s_begin; s0 < s_end; s0 += 2) {
            const size_t s = s0 + half;
            float av = 0.0f, vr = 0.0f, vu = 0.0f, vc = 0.0f;
            if (s < s_end) {
                vr = br[s]; vu = bu[s]; vc = bc[s];
                const bool st = s < n || a.start[s];
                if (ta < NXB) {
                    av = x(a, 32 * ta + i, s, st);
                } else {
                    const int k = 32 * (ta - NXB) + i;
                    av = st ? a.theta[k] : a.hs[(size_t)k * B + s - n];
                }
            }
            cr = mfma(av, vr, cr); cu = mfma(av, vu, cu); cc = mfma(av, vc, cc);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int c = 32 * jb + i;
            if (ta < NXB) {
                const int row = 32 * ta + frag_unit(r, half);
                if (row < DI) {
                    out[off.wx(0) + row * H + c] = cr[r]; out[off.wx(1) + row * H + c] = cu[r];
                    out[off.wx(2) + row * H + c] = cc[r];
                } else if (row == DI) {
                    out[off.b(0, DI) + c] = cr[r]; out[off.b(1, DI) + c] = cu[r]; out[off.b(2, DI) + c] = cc[r];
                }
            } else {
                const int k = 32 * (ta - NXB) + frag_unit(r, half);
                out[off.wh(0, DI) + k * H + c] = cr[r]; out[off.wh(1, DI) + k * H + c] = cu[r];
                out[off.wh(2, DI) + k * H + c] = cc[r];
            }
        }
    } else {
        const int q = job - (NXB + NB) * NB;
        const float* hrow = a.hs + (size_t)(32 * q + i) * B;
        const float* dcol = a.dmean + (size_t)(i < NOUT ? i : 0) * B;
        f32x16 acc = {0};
        for (size_t s0 = s_begin; s0 < s_end; s0 += 2) {
            const size_t s = s0 + half;
            float av = 0.0f, bv = 0.0f;
            if (s < s_end) { av = hrow[s]; bv = i < NOUT ? dcol[s] : 0.0f; }
            acc = mfma(av, bv, acc);
        }
        if (i < NOUT) {
#pragma unroll
            for (int r = 0; r < 16; ++r) out[off.w_out + (32 * q + frag_unit(r, half)) * NOUT + i] = acc[r];
        }
    }
}

// The results from the partial sums, each added in index order.  mode 0: loss and KL; 1: and the gradient; 2: F v.
// n_ls: the log-std rows behind b_out (the Gaussian family's; 0: none).
template <class Dev>
__global__ void __launch_bounds__(256) gru_finish_kernel(Dev a, int H, int NOUT, int n_ls, int DI, int P4, int chunks,
                                                         int blocks, int mode, double* out2, float* grad) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p == 0 && out2) {
        double loss = 0.0, kl = 0.0;
        for (int b = 0; b < blocks; ++b) { loss += a.part[(size_t)b * BPTT_PART]; kl += a.part[(size_t)b * BPTT_PART + 1]; }
        out2[0] = loss * a.inv_count; out2[1] = kl * a.inv_count;
    }
    const int w_out = H + 3 * (DI * H + H * H + H), b_out = w_out + H * NOUT, total = b_out + NOUT;
    if (mode == 0 || p >= total + n_ls) return;
    float g = 0.0f;                                       // h0 is not trainable
    if (p >= H && p < b_out) {
        for (int c = 0; c < chunks; ++c) g += a.wpart[(size_t)c * P4 + p];
    } else if (p >= b_out) {
        const int k = p < total ? p - b_out : p - total, slot = p < total ? 3 + 8 + k : 3 + k;
        double sum = 0.0;
        for (int b = 0; b < blocks; ++b) sum += a.part[(size_t)b * BPTT_PART + (mode == 2 && p >= total ? 2 : slot)];
        if (mode == 2 && p >= total) {
            // d^2 / d log_std^2 of the KL's  (so^2 - q) / (2 q + eps) + log_std  at  q = sigma^2 = so^2: 4 q (2 q - eps) / (2 q + eps)^2
            const double sg = sigma_of(a.theta[p]), q2 = 2.0 * sg * sg;
            sum = 2.0 * q2 * (q2 - 1e-8) / ((q2 + 1e-8) * (q2 + 1e-8)) * (double)a.v[p] * sum * a.inv_count;
        }
        g = (float)sum;
    }
    grad[p] = g;
}

// ---- host ------------------------------------------------------------------------------------------------------------

struct BpttPlan {
    int H, DO, DA, DI, P, P4, blocks, chunks, L;
    size_t B, bytes, o_part, o_hs, o_d[4], o_dmean, o_wpart;
};

inline size_t bptt_up16(size_t b) { return (b + 15) & ~(size_t)15; }

// bytes of LDS of the larger of the two sweeps -- the tangent sweep: theta, v and three tiles; the backward sweep: theta
// and five tiles -- for P4 staged parameters
inline size_t bptt_lds_bytes(int hidden, int P4) {
    const size_t tile = (size_t)hidden * WV, fvp = 2 * (size_t)P4 + 3 * tile, bwd = (size_t)P4 + 5 * tile;
    return (fvp > bwd ? fvp : bwd) * sizeof(float);
}

// the sample chunks of the weight sums and the workspace of a plan whose H, DA (the number of outputs) and P4 are set
inline void bptt_workspace(BpttPlan& p, long long n, long long T) {
    p.B = (size_t)(n * T);
    p.blocks = (int)((n + GRU_BLOCK - 1) / GRU_BLOCK);
    const size_t chunks = (p.B + 127) / 128;
    p.chunks = (int)(chunks < (size_t)BPTT_MAX_CHUNKS ? chunks : (size_t)BPTT_MAX_CHUNKS);
    p.L = (int)(2 * ((p.B + 2 * (size_t)p.chunks - 1) / (2 * (size_t)p.chunks)));
    const size_t plane = bptt_up16(p.B * sizeof(float));
    size_t o = 0;
    p.o_part = o; o += bptt_up16((size_t)p.blocks * BPTT_PART * sizeof(double));
    p.o_hs = o; o += plane * p.H;
    for (int k = 0; k < 4; ++k) { p.o_d[k] = o; o += plane * p.H; }
    p.o_dmean = o; o += plane * p.DA;
    p.o_wpart = o; o += (size_t)p.chunks * p.P4 * sizeof(float);
    p.bytes = o;
}

// the workspace pointers of a plan into a Dev
template <class Dev>
inline void bptt_bind_workspace(Dev& a, const BpttPlan& p, void* workspace) {
    char* ws = (char*)workspace;
    a.part = (double*)(ws + p.o_part); a.hs = (float*)(ws + p.o_hs);
    a.dr = (float*)(ws + p.o_d[0]); a.du = (float*)(ws + p.o_d[1]); a.dc = (float*)(ws + p.o_d[2]);
    a.rdc = (float*)(ws + p.o_d[3]); a.dmean = (float*)(ws + p.o_dmean); a.wpart = (float*)(ws + p.o_wpart);
}

// behind the sweep of a gradient or product pass (mode 1, 2): the backward sweep and the weight sums; then, for every
// mode, the finish.  n_ls: the family's rows behind GruLayout's total.
template <class In, int NOUT, int H, class Dev, class Rows, class Refuse>
static int bptt_run_tail(const Dev& a, const BpttPlan& p, const Rows& x, int n_ls, int mode, double* out2, float* grad,
                         hipStream_t st, Refuse refuse) {
    int rc;
    if (mode != 0) {
        rc = launch_gru_lanes<gru_bwd_kernel<In, NOUT, H, Dev>, H, NOUT>("gru_bwd_kernel", a, a.n, p.DI, n_ls + 3 * H * WV, st,
                                                                          refuse);
        if (rc) return rc;
        const int NB = H / 32;
        const dim3 grid((unsigned)p.chunks, (unsigned)((bptt_input_blocks(p.DI) + NB) * NB + NB));
        hipLaunchKernelGGL((gru_wgrad_kernel<H, Rows, Dev>), grid, dim3(WV), 0, st, a, x, NOUT, p.P4, p.L);
        rc = check_launch("gru_wgrad_kernel");
        if (rc) return rc;
    }
    const int threads = mode == 0 ? 1 : p.P;
    hipLaunchKernelGGL(gru_finish_kernel<Dev>, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, a, H, NOUT, n_ls,
                       p.DI, p.P4, p.chunks, p.blocks, mode, out2, grad);
    return check_launch("gru_finish_kernel");
}

}  // namespace rl
