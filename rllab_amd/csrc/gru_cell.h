// gru_cell.h -- the one GRU step (rllab/core/network.py:150-155) of the env-per-lane recurrent rollouts, and what they do
// around it.  Shared by gru_kernels.hip (dense input, Env::ACT means), categorical_gru_kernels.hip (one-hot input, four
// logits) and population_gru_kernels.hip (dense input, every lane its own weights).
//
// Weights: the step takes them from a SOURCE, addressed by their offset (in floats) inside the parameter vector, four
// consecutive ones per read.  LdsWeights: the same for every lane, staged ONCE per workgroup into LDS in the order they
// arrive in and read at lane-uniform addresses (every lane the same address: one broadcast, no bank conflict), four output
// units per 16-byte read.  RowWeights: one parameter vector per lane, read from the transposed population image
// theta_pop_T[P][n_cand] -- entry e of every candidate is row e, so a read of the wavefront is one coalesced row segment.
// The hidden state lives in LDS, as two [H][64] tiles (lane l only ever touches column l: no bank conflict, no
// synchronisation): a step reads all of h from one tile while it writes h' into the other, then they swap.  The unit loop
// runs at run time over blocks of GRU_UB units whose accumulators are named registers -- no register array is indexed at
// run time, nothing of the policy is alive while an env steps.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include "capi_util.h"
#include "policy_mfma.h"
#include "population_lane.h"

namespace rl {

constexpr int GRU_BLOCK = 64;   // one wavefront per workgroup, one env per lane
constexpr int GRU_UB = 4;       // hidden units evaluated together: one 16-byte weight read per gate and input row
constexpr double GRU_LDS_LIMIT = 160 * 1024;

// offsets (in floats) of the parameter vector for input width DI: h0 [H], then per gate W_x [DI][H], W_h [H][H], b [H]
// for r, u, c, then W_out [H][NOUT], b_out [NOUT]; `total` is where a caller's own rows (the Gaussian log-std) follow
template <int H, int NOUT>
struct GruLayout {
    int gate, w_out, b_out, total;
    __host__ __device__ explicit GruLayout(int DI) {
        gate = DI * H + H * H + H;
        w_out = H + 3 * gate;
        b_out = w_out + H * NOUT;
        total = b_out + NOUT;
    }
    __host__ __device__ int wx(int g) const { return H + g * gate; }
    __host__ __device__ int wh(int g, int DI) const { return wx(g) + DI * H; }
    __host__ __device__ int b(int g, int DI) const { return wh(g, DI) + H * H; }
};

__device__ __forceinline__ float fsigmoid(float z) {       // 1 / (1 + exp(-z))
    return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(z * -1.4426950408889634f));
}

struct F4 { float v[GRU_UB]; };
__device__ __forceinline__ F4 lds4(const float* p) {       // 16-byte aligned by construction: every row is H floats
    const float4 q = *reinterpret_cast<const float4*>(p);
    return F4{{q.x, q.y, q.z, q.w}};
}

// the staged parameter vector in LDS, the same for every lane
struct LdsWeights {
    static constexpr int K_BLOCK = 1;         // hidden rows read ahead of their FMAs: an LDS broadcast is there at once
    const float* w;
    __device__ __forceinline__ F4 load4(int e) const { return lds4(w + e); }      // e a multiple of 4
    __device__ __forceinline__ float load(int e) const { return w[e]; }
};

// this lane's column of theta_pop_T[P][n_cand]: entries e .. e + 3 are four consecutive rows (RowWalk: scalar row base +
// the lane's 32-bit byte offset)
struct RowWeights {
    // hidden rows read ahead of their FMAs: a wavefront has its SIMD to itself and a row read comes from the memory side,
    // so the 3 * GRU_UB * K_BLOCK reads of a block are all in flight before the first FMA waits for one
    static constexpr int K_BLOCK = 8;
    const float* theta_T;
    size_t row_bytes;
    mutable uint32_t lane_bytes;              // (RowWalk pins it to a vector register: not a value that changes)
    __device__ __forceinline__ F4 load4(int e) const {
        RowWalk r(theta_T, row_bytes, e);
        F4 q;
#pragma unroll
        for (int u = 0; u < GRU_UB; ++u) q.v[u] = r.next(row_bytes, lane_bytes);
        return q;
    }
    __device__ __forceinline__ float load(int e) const { return RowWalk(theta_T, row_bytes, e).next(row_bytes, lane_bytes); }
};

// x W_x* of a dense x = [o, prev_action]: float32 FMAs in the order of the input index
template <int DO, int DA, int H>
struct DenseInput {
    const float* o;
    const float* pa;
    bool include_action;
    template <class W>
    __device__ __forceinline__ void row(const W& w, float x, int d, int xr, int xu, int xc, int j, F4& ar, F4& au,
                                        F4& ax) const {
        const F4 wr = w.load4(xr + d * H + j), wu = w.load4(xu + d * H + j), wc = w.load4(xc + d * H + j);
#pragma unroll
        for (int u = 0; u < GRU_UB; ++u) {
            ar.v[u] = __builtin_fmaf(x, wr.v[u], ar.v[u]);
            au.v[u] = __builtin_fmaf(x, wu.v[u], au.v[u]);
            ax.v[u] = __builtin_fmaf(x, wc.v[u], ax.v[u]);
        }
    }
    template <class W>
    __device__ __forceinline__ void operator()(const W& w, int xr, int xu, int xc, int j, F4& ar, F4& au, F4& ax) const {
#pragma unroll
        for (int d = 0; d < DO; ++d) row(w, o[d], d, xr, xu, xc, j, ar, au, ax);
        if (include_action) {
#pragma unroll
            for (int d = 0; d < DA; ++d) row(w, pa[d], DO + d, xr, xu, xc, j, ar, au, ax);
        }
    }
};

// x W_x* of x = [onehot(s), onehot(pa)] over S states: a ROW READ per one -- row s, then row S + pa unless pa < 0 (a path
// start, or a policy that does not see its previous action).  The only LDS reads at lane-varying addresses.
template <int H>
struct OneHotInput {
    int row_s, row_a, pa;
    __device__ __forceinline__ OneHotInput(int S, int s, int pa_)
        : row_s(s * H), row_a((S + (pa_ < 0 ? 0 : pa_)) * H), pa(pa_) {}     // row_a: only read when pa >= 0
    static __device__ __forceinline__ void add(F4& a, const F4& b) {
#pragma unroll
        for (int u = 0; u < GRU_UB; ++u) a.v[u] = a.v[u] + b.v[u];
    }
    template <class W>
    __device__ __forceinline__ void operator()(const W& w, int xr, int xu, int xc, int j, F4& ar, F4& au, F4& ax) const {
        add(ar, w.load4(xr + row_s + j));
        add(au, w.load4(xu + row_s + j));
        add(ax, w.load4(xc + row_s + j));
        if (pa >= 0) {
            add(ar, w.load4(xr + row_a + j));
            add(au, w.load4(xu + row_a + j));
            add(ax, w.load4(xc + row_a + j));
        }
    }
};

// one GRU step of this lane: reads h from column `hc`, writes h' into column `hn`, returns out = h' W_out + b_out.
// w: where the weights come from (LdsWeights, RowWeights), addressed by their offset inside the parameter vector.
// input(w, xr, xu, xc, j, ar, au, ax) adds x W_x* of units j .. j + GRU_UB into the three gate sums, behind the biases and
// ahead of the hidden units, which follow in index order.
template <int H, int NOUT, class W, class Input>
__device__ __forceinline__ void gru_cell(const W& w, const GruLayout<H, NOUT>& off, int DI, const Input& input,
                                         const float* hc, float* hn, float* out) {
    static_assert(H % GRU_UB == 0, "unit blocks");
#pragma unroll
    for (int k = 0; k < NOUT; ++k) out[k] = w.load(off.b_out + k);
    const int xr = off.wx(0), hr = off.wh(0, DI), br = off.b(0, DI);
    const int xu = off.wx(1), hu = off.wh(1, DI), bu = off.b(1, DI);
    const int xc = off.wx(2), hcw = off.wh(2, DI), bc = off.b(2, DI);
    const int wo = off.w_out;
#pragma unroll 1
    for (int j = 0; j < H; j += GRU_UB) {
        F4 ar = w.load4(br + j), au = w.load4(bu + j), ax = w.load4(bc + j), ah = F4{{0.0f, 0.0f, 0.0f, 0.0f}};
        input(w, xr, xu, xc, j, ar, au, ax);
        constexpr int KB = W::K_BLOCK;            // rows read together; the FMAs follow in index order either way
        static_assert(8 % KB == 0 && H % 8 == 0, "row blocks");
#pragma unroll(8 / KB)
        for (int k0 = 0; k0 < H; k0 += KB) {
            float hk[KB];
            F4 wr[KB], wu[KB], wc[KB];
#pragma unroll
            for (int q = 0; q < KB; ++q) {
                const int k = k0 + q;
                hk[q] = hc[k * WV];
                wr[q] = w.load4(hr + k * H + j); wu[q] = w.load4(hu + k * H + j); wc[q] = w.load4(hcw + k * H + j);
            }
#pragma unroll
            for (int q = 0; q < KB; ++q) {
                const float h = hk[q];
#pragma unroll
                for (int u = 0; u < GRU_UB; ++u) {
                    ar.v[u] = __builtin_fmaf(h, wr[q].v[u], ar.v[u]);
                    au.v[u] = __builtin_fmaf(h, wu[q].v[u], au.v[u]);
                    ah.v[u] = __builtin_fmaf(h, wc[q].v[u], ah.v[u]);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < GRU_UB; ++u) {
            const float r = fsigmoid(ar.v[u]), g = fsigmoid(au.v[u]);
            const float c = ftanh(__builtin_fmaf(r, ah.v[u], ax.v[u]));
            const float h_old = hc[(j + u) * WV];
            const float h_new = __builtin_fmaf(g, c, (1.0f - g) * h_old);
            hn[(j + u) * WV] = h_new;
            if constexpr (NOUT == GRU_UB) {                   // W_out[j + u][:] is one 16-byte read
                const F4 q = w.load4(wo + (j + u) * NOUT);
#pragma unroll
                for (int k = 0; k < NOUT; ++k) out[k] = __builtin_fmaf(h_new, q.v[k], out[k]);
            } else {
#pragma unroll
                for (int k = 0; k < NOUT; ++k) out[k] = __builtin_fmaf(h_new, w.load(wo + (j + u) * NOUT + k), out[k]);
            }
        }
    }
}

// This lane's column of the two [H][64] hidden-state tiles.
template <int H>
struct GruTiles {
    float* hc;          // column of the tile that holds h, what the next step reads
    float* hn;          // column of the tile the next step writes
    template <class W>
    __device__ __forceinline__ void fill_h0(const W& w) {       // h0: the first H entries of the parameter vector
#pragma unroll 1
        for (int k = 0; k < H; ++k) hc[k * WV] = w.load(k);
    }
    __device__ __forceinline__ void swap() { float* sw = hc; hc = hn; hn = sw; }
};

// This lane's view of the workgroup's dynamic LDS: the staged parameters and its column of the two hidden-state tiles.
template <int H>
struct GruLanes : GruTiles<H> {
    using GruTiles<H>::hc;
    using GruTiles<H>::hn;
    const float* w;     // [w_floats]: theta, the same for every lane
    // every thread of the workgroup, before any of them leaves: stages theta[0 .. n_theta) and synchronises.
    // w_floats >= n_theta, a multiple of 4 (the tiles behind it stay 16-byte aligned).
    __device__ __forceinline__ GruLanes(const float* theta, int n_theta, int w_floats) {
        extern __shared__ __attribute__((aligned(16))) float gru_smem[];
        for (int e = threadIdx.x; e < n_theta; e += GRU_BLOCK) gru_smem[e] = theta[e];
        __syncthreads();
        w = gru_smem;
        hc = gru_smem + w_floats + threadIdx.x;
        hn = hc + H * WV;
    }
    __device__ __forceinline__ void fill_h0() { GruTiles<H>::fill_h0(LdsWeights{w}); }
    __device__ __forceinline__ void load(const float* plane, int n, int i) {      // plane [H][n]
#pragma unroll 1
        for (int k = 0; k < H; ++k) hc[k * WV] = plane[(size_t)k * n + i];
    }
    __device__ __forceinline__ void store(float* plane, int n, int i) const {
#pragma unroll 1
        for (int k = 0; k < H; ++k) plane[(size_t)k * n + i] = hc[k * WV];
    }
};

// Launch `Kern(args, w_floats)`, one workgroup per 64 envs, with the LDS of a GruLayout<H, NOUT>(DI) + `extra` floats and
// the two tiles.  The byte count is taken in double: exact up to 2^53, so an input width that does not fit an int is
// refused before it is used as one.  refuse(bytes) makes the entry point's error of a request above the LDS of a CU.
template <auto Kern, int H, int NOUT, class Args, class Refuse>
static int launch_gru_lanes(const char* kernel_name, const Args& a, int n_envs, long long DI, int extra, hipStream_t st,
                            Refuse refuse) {
    const double floats = (double)H + 3.0 * ((double)DI * H + (double)H * H + H) + (double)H * NOUT + NOUT + extra;
    const double need = (4.0 * ceil(floats / 4.0) + 2.0 * H * WV) * sizeof(float);
    if (need > GRU_LDS_LIMIT) return refuse(need);
    const int w_floats = (GruLayout<H, NOUT>((int)DI).total + extra + 3) & ~3;
    const size_t lds = (size_t)need;
    static size_t attr_lds = 0;                 // per kernel instantiation: the largest request so far
    if (lds > attr_lds) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(Kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)lds);
        if (e != hipSuccess) return set_error(RL_ERR_HIP, "hipFuncSetAttribute: %s", hipGetErrorString(e));
        attr_lds = lds;
    }
    const dim3 grid((unsigned)((n_envs + GRU_BLOCK - 1) / GRU_BLOCK)), block(GRU_BLOCK);
    hipLaunchKernelGGL(Kern, grid, block, lds, st, a, w_floats);
    return check_launch(kernel_name);
}

}  // namespace rl
