// gru_bptt.h -- what the update kernels of a GaussianGRUPolicy (gru_bptt_kernels.hip) need next to the GRU step of
// gru_cell.h: the gate sums of one block of units on their own, and the batch as the sweeps see it.
//
// gru_cell evaluates a whole step and keeps the gates to itself; the backward sweep and the tangent sweep need r, u, c
// and h W_hc of the step they are at.  gru_preact4 / gru_hidden4 RESTATE the sums of gru_cell -- bias, then the inputs,
// then the hidden units, each in index order, one float32 FMA per term -- so a gate recomputed here from the h the
// forward sweep stored is the gate the forward sweep used, bit for bit.  gru_cell itself is left as it is: three rollout
// kernels are pinned to its instruction stream.
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

// A recurrent batch on its dense planes (sample s = t * n + i of env column i) and the workspace of its update passes.
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
    float* dmean;               // [DA][B] cotangent of the means
    float* wpart;               // [chunks][P4] the weight gradient's partial sums
};

}  // namespace rl
