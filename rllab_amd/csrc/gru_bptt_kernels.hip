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

// sigma of a log-std row entry, in float64 from the float32 value (new and old the same expression: their difference
// vanishes identically at equal inputs)
__device__ __forceinline__ double sigma_of(float log_std) { return exp((double)log_std); }

template <int DA>
__device__ __forceinline__ void write_partials(const BpttDev& a, double loss, double kl, double sw, const double* dls,
                                               const double* dbo) {
    double* p = a.part + (size_t)blockIdx.x * BPTT_PART;
    loss = wave_sum(loss); kl = wave_sum(kl); sw = wave_sum(sw);
    if (threadIdx.x == 0) { p[0] = loss; p[1] = kl; p[2] = sw; }
#pragma unroll
    for (int k = 0; k < DA; ++k) {
        const double l = wave_sum(dls[k]), b = wave_sum(dbo[k]);
        if (threadIdx.x == 0) { p[3 + k] = l; p[3 + 8 + k] = b; }
    }
}

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
            const DenseInput<DO, DA, H> in{o, pa, a.include_action != 0};
#pragma unroll 1
            for (int j = 0; j < H; j += GRU_UB) {
                F4 ar, au, ax, ah, tr, tu, tx, tah;
                gru_preact4(th, off, DI, in, hp, j, ar, au, ax, ah);
                gru_preact4(vw, off, DI, in, hp, j, tr, tu, tx, tah);       // the weights move ...
                gru_hidden4(th, off, DI, lanes.hc, j, tr, tu, tah);         // ... and so does h
#pragma unroll
                for (int u = 0; u < GRU_UB; ++u) {
                    const float r = fsigmoid(ar.v[u]), g = fsigmoid(au.v[u]);
                    const float c = ftanh(__builtin_fmaf(r, ah.v[u], ax.v[u]));
                    const float h_old = hp[(j + u) * WV];
                    const float h_new = __builtin_fmaf(g, c, (1.0f - g) * h_old);
                    const float dr = r * (1.0f - r) * tr.v[u], dg = g * (1.0f - g) * tu.v[u];
                    const float dc = (1.0f - c * c) * (tx.v[u] + dr * ah.v[u] + r * tah.v[u]);
                    const float dh = dg * (c - h_old) + g * dc + (1.0f - g) * lanes.hc[(j + u) * WV];
                    lanes.hn[(j + u) * WV] = dh;
#pragma unroll
                    for (int k = 0; k < DA; ++k) {
                        tm[k] = __builtin_fmaf(dh, th.load(off.w_out + (j + u) * DA + k), tm[k]);
                        tm[k] = __builtin_fmaf(h_new, vw.load(off.w_out + (j + u) * DA + k), tm[k]);
                    }
                }
            }
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

// LDS: theta [P4], the tiles of dr, du and r * dc of the step, then h_prev and dh (GruLanes' hc / hn).
template <int DO, int DA, int H>
__global__ void __launch_bounds__(GRU_BLOCK) gru_bwd_kernel(BpttDev a, int w_floats) {
    const int DI = DO + (a.include_action ? DA : 0);
    const GruLayout<H, DA> off(DI);
    const int n_theta = off.total + DA, P4 = (n_theta + 3) & ~3;
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
        float pa[DA], o[DO], dm[DA];
        if (t == 0 || a.start[s]) {
#pragma unroll 1
            for (int k = 0; k < H; ++k) hp[k * WV] = th.load(k);
#pragma unroll
            for (int k = 0; k < DA; ++k) pa[k] = 0.0f;
        } else {
#pragma unroll 4
            for (int k = 0; k < H; ++k) hp[k * WV] = a.hs[(size_t)k * B + s - a.n];
#pragma unroll
            for (int k = 0; k < DA; ++k) pa[k] = a.actions[(size_t)k * B + s - a.n];
        }
#pragma unroll
        for (int d = 0; d < DO; ++d) o[d] = a.obs[(size_t)d * B + s];
#pragma unroll
        for (int k = 0; k < DA; ++k) dm[k] = a.dmean[(size_t)k * B + s];
        const DenseInput<DO, DA, H> in{o, pa, a.include_action != 0};
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
                for (int k = 0; k < DA; ++k) d = __builtin_fmaf(dm[k], th.load(off.w_out + (j + u) * DA + k), d);
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

// One wavefront: the sums over the samples [c L, (c + 1) L) of one 32-row block of [x; 1] or of h_prev against one
// 32-column block of dr, du, dc (r dc for h_prev) -- three 32 x 32 tiles -- or of 32 units of h' against dmean.
// MFMA operands (v_mfma_f32_32x32x2_f32): lane l holds row l & 31 of the left factor and column l & 31 of the right one
// at sample s0 + (l >> 5); the result's column is l & 31, its rows frag_unit(register, l >> 5).
template <int H>
__global__ void __launch_bounds__(WV) gru_wgrad_kernel(BpttDev a, int DO, int DA, int DI, int P4, int L) {
    constexpr int NB = H / 32;
    const GruLayout<H, 1> off(DI);            // (the offsets used here do not depend on the number of outputs)
    const int l = threadIdx.x, i = l & 31, half = l >> 5, job = blockIdx.y;
    const size_t B = a.B, n = (size_t)a.n;
    const size_t s_begin = (size_t)blockIdx.x * L, s_end = s_begin + L < B ? s_begin + L : B;
    float* out = a.wpart + (size_t)blockIdx.x * P4;
    if (job < (1 + NB) * NB) {
        const int ta = job / NB, jb = job % NB;
        const size_t col = (size_t)(32 * jb + i) * B;
        const float* br = a.dr + col;
        const float* bu = a.du + col;
        const float* bc = (ta == 0 ? a.dc : a.rdc) + col;
        f32x16 cr = {0}, cu = {0}, cc = {0};
        for (size_t s0 = s_begin; s0 < s_end; s0 += 2) {
            const size_t s = s0 + half;
            float av = 0.0f, vr = 0.0f, vu = 0.0f, vc = 0.0f;
            if (s < s_end) {
                vr = br[s]; vu = bu[s]; vc = bc[s];
                const bool st = s < n || a.start[s];
                if (ta == 0) {
                    if (i < DO) av = a.obs[(size_t)i * B + s];
                    else if (i < DI) av = st ? 0.0f : a.actions[(size_t)(i - DO) * B + s - n];
                    else if (i == DI) av = 1.0f;
                } else {
                    const int k = 32 * (ta - 1) + i;
                    av = st ? a.theta[k] : a.hs[(size_t)k * B + s - n];
                }
            }
            cr = mfma(av, vr, cr); cu = mfma(av, vu, cu); cc = mfma(av, vc, cc);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = frag_unit(r, half), c = 32 * jb + i;
            if (ta == 0) {
                if (row < DI) {
                    out[off.wx(0) + row * H + c] = cr[r]; out[off.wx(1) + row * H + c] = cu[r];
                    out[off.wx(2) + row * H + c] = cc[r];
                } else if (row == DI) {
                    out[off.b(0, DI) + c] = cr[r]; out[off.b(1, DI) + c] = cu[r]; out[off.b(2, DI) + c] = cc[r];
                }
            } else {
                const int k = 32 * (ta - 1) + row;
                out[off.wh(0, DI) + k * H + c] = cr[r]; out[off.wh(1, DI) + k * H + c] = cu[r];
                out[off.wh(2, DI) + k * H + c] = cc[r];
            }
        }
    } else {
        const int q = job - (1 + NB) * NB;
        const float* hrow = a.hs + (size_t)(32 * q + i) * B;
        const float* dcol = a.dmean + (size_t)(i < DA ? i : 0) * B;
        f32x16 acc = {0};
        for (size_t s0 = s_begin; s0 < s_end; s0 += 2) {
            const size_t s = s0 + half;
            float av = 0.0f, bv = 0.0f;
            if (s < s_end) { av = hrow[s]; bv = i < DA ? dcol[s] : 0.0f; }
            acc = mfma(av, bv, acc);
        }
        if (i < DA) {
#pragma unroll
            for (int r = 0; r < 16; ++r) out[off.w_out + (32 * q + frag_unit(r, half)) * DA + i] = acc[r];
        }
    }
}

// The results from the partial sums, each added in index order.  mode 0: loss and KL; 1: and the gradient; 2: F v.
__global__ void __launch_bounds__(256) gru_finish_kernel(BpttDev a, int H, int DA, int DI, int P4, int chunks, int blocks,
                                                         int mode, double* out2, float* grad) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p == 0 && out2) {
        double loss = 0.0, kl = 0.0;
        for (int b = 0; b < blocks; ++b) { loss += a.part[(size_t)b * BPTT_PART]; kl += a.part[(size_t)b * BPTT_PART + 1]; }
        out2[0] = loss * a.inv_count; out2[1] = kl * a.inv_count;
    }
    const int w_out = H + 3 * (DI * H + H * H + H), b_out = w_out + H * DA, total = b_out + DA;
    if (mode == 0 || p >= total + DA) return;
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

static size_t up16(size_t b) { return (b + 15) & ~(size_t)15; }

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
    // the tangent sweep: theta, v and three tiles; the backward sweep: theta and five tiles
    const size_t tile = (size_t)hidden * WV, fvp = 2 * (size_t)p.P4 + 3 * tile, bwd = (size_t)p.P4 + 5 * tile;
    const size_t need = (fvp > bwd ? fvp : bwd) * sizeof(float);
    if ((double)need > GRU_LDS_LIMIT)
        return set_error(RL_ERR_UNSUPPORTED, "%s: %zu bytes of LDS for the weights, the tangent vector and the state tiles "
                         "of %d hidden units on %d inputs (a CU has 160 KB)", fn, need, hidden, p.DI);
    p.B = (size_t)(n * T);
    p.blocks = (int)((n + GRU_BLOCK - 1) / GRU_BLOCK);
    const size_t chunks = (p.B + 127) / 128;
    p.chunks = (int)(chunks < (size_t)BPTT_MAX_CHUNKS ? chunks : (size_t)BPTT_MAX_CHUNKS);
    p.L = (int)(2 * ((p.B + 2 * (size_t)p.chunks - 1) / (2 * (size_t)p.chunks)));
    const size_t plane = up16(p.B * sizeof(float));
    size_t o = 0;
    p.o_part = o; o += up16((size_t)p.blocks * BPTT_PART * sizeof(double));
    p.o_hs = o; o += plane * hidden;
    for (int k = 0; k < 4; ++k) { p.o_d[k] = o; o += plane * hidden; }
    p.o_dmean = o; o += plane * act_dim;
    p.o_wpart = o; o += (size_t)p.chunks * p.P4 * sizeof(float);
    p.bytes = o;
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
    if (mode != 0) {
        rc = launch_gru_lanes<gru_bwd_kernel<DO, DA, H>, H, DA>("gru_bwd_kernel", a, a.n, p.DI, DA + 3 * tile, st, refuse);
        if (rc) return rc;
        const dim3 grid((unsigned)p.chunks, (unsigned)((1 + H / 32) * (H / 32) + H / 32));
        hipLaunchKernelGGL(gru_wgrad_kernel<H>, grid, dim3(WV), 0, st, a, DO, DA, p.DI, p.P4, p.L);
        rc = check_launch("gru_wgrad_kernel");
        if (rc) return rc;
    }
    const int threads = mode == 0 ? 1 : p.P;
    hipLaunchKernelGGL(gru_finish_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, a, H, DA, p.DI, p.P4,
                       p.chunks, p.blocks, mode, out2, grad);
    return check_launch("gru_finish_kernel");
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
    char* ws = (char*)b->workspace;
    BpttDev a;
    a.n = b->n_envs; a.T = b->horizon; a.include_action = b->include_action; a.B = p.B; a.inv_count = b->inv_count;
    a.theta = b->theta; a.v = v; a.obs = b->obs; a.actions = b->actions; a.adv = b->advantages;
    a.old_means = b->old_means; a.old_log_std = b->old_log_std; a.weights = b->weights; a.start = b->start;
    a.means = mode == 2 ? nullptr : b->means;
    a.part = (double*)(ws + p.o_part); a.hs = (float*)(ws + p.o_hs);
    a.dr = (float*)(ws + p.o_d[0]); a.du = (float*)(ws + p.o_d[1]); a.dc = (float*)(ws + p.o_d[2]);
    a.rdc = (float*)(ws + p.o_d[3]); a.dmean = (float*)(ws + p.o_dmean); a.wpart = (float*)(ws + p.o_wpart);
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
