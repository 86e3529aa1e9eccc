// cmaes_kernels.hip -- the covariance update of CMA-ES (rllab/algos/cma_es_lib.py:3800-3814, full-matrix case with the
// active / negative accumulator) as ONE pass over the N x N float64 state:
//
//   _Yneg[i][j] <- s2 * _Yneg[i][j] + sum_k wneg[k] Vneg[k][i] Vneg[k][j] - C_old[i][j]          (s2 = 1 - cmuexp)
//   C[i][j]     <- s0 * C_old[i][j] + sum_k wpos[k] Ypos[k][i] Ypos[k][j] + s1 * pc[i] pc[j]     (s0 = 1 - c1a - cmu, s1 = c1)
//   dC[i]       <- C[i][i]
//
// s0, s1, s2 come from a float64 block in DEVICE memory: c1a depends on hsig, a device value of the same iteration, and
// nothing is read back in front of the launch.  C_old and _Yneg are read once and written once (4 N^2 8 B of traffic for
// about 2 N^2 (mu + mu_neg + 1) flops: memory-bound by a wide margin at the ranks CMA-ES uses), so the sums run on plain
// float64 vector FMAs, not on the matrix pipe.
//
// Tile: a workgroup of 256 threads owns 32 rows x 64 columns.  Wavefront w owns rows 8w .. 8w+7 of the tile, lane l column
// l: every global access of a wavefront is one 512-byte row segment.  Per chunk of CM_KC ranks the tile's slices of the
// rank vectors are staged in LDS, Yi[k][32] (row side) and Yj[k][64] (column side): the column read is lane l at 8 l bytes
// (two 32-lane groups on 64 distinct banks, conflict-free), the 8 row reads are one 64-byte block every lane of the
// wavefront reads alike (broadcast).  Any mu / mu_neg: the chunk loop, not the LDS size, bounds them.
//
// Summation order is fixed: ranks ascending, every term as fma(w_k, round(a_i * a_j), acc), the rank-one term last.  The
// product a_i * a_j is rounded BEFORE the weight goes in, so entry (i, j) and entry (j, i) are the same sequence of
// operations on the same numbers: with symmetric C_old and _Yneg the result is exactly symmetric, and two launches on equal
// inputs give equal bits (no atomics, no order that depends on the launch).
#include <hip/hip_runtime.h>
#include <math.h>
#include "../../include/rllab_amd.h"
#include "capi_util.h"

namespace rl {

constexpr int CM_TI = 32;              // tile rows
constexpr int CM_TJ = 64;              // tile columns = lanes
constexpr int CM_RPT = 8;              // rows per thread (CM_TI / 4 wavefronts)
constexpr int CM_KC = 32;              // ranks staged per chunk: 32 * (32 + 64 + 1) * 8 B = 24.25 KiB of LDS

struct alignas(16) CmTileLds {
    double yi[CM_KC][CM_TI];
    double yj[CM_KC][CM_TJ];
    double w[CM_KC];
};

// acc[r] += sum_k w[k] * (Y[k][i0 + row(r)] * Y[k][j]), k ascending over all `rank` rows of Y [rank][N]
__device__ __forceinline__ void cm_accumulate(CmTileLds& s, const double* __restrict__ Y, const double* __restrict__ wgt,
                                              int rank, int N, int i0, int j0, int tid, int wv, int lane,
                                              double (&acc)[CM_RPT]) {
    for (int k0 = 0; k0 < rank; k0 += CM_KC) {
        const int kc = min(CM_KC, rank - k0);
        __syncthreads();                                   // the previous chunk (or phase) has been consumed
        for (int e = tid; e < kc * CM_TJ; e += 256) {
            const int k = e / CM_TJ, c = e % CM_TJ, j = j0 + c;
            s.yj[k][c] = j < N ? Y[(size_t)(k0 + k) * N + j] : 0.0;
        }
        for (int e = tid; e < kc * CM_TI; e += 256) {
            const int k = e / CM_TI, r = e % CM_TI, i = i0 + r;
            s.yi[k][r] = i < N ? Y[(size_t)(k0 + k) * N + i] : 0.0;
        }
        if (tid < kc) s.w[tid] = wgt[k0 + tid];
        __syncthreads();
        for (int k = 0; k < kc; ++k) {
            const double yj = s.yj[k][lane];
            const double wk = s.w[k];
#pragma unroll
            for (int r = 0; r < CM_RPT; ++r) {
                const double p = __dmul_rn(s.yi[k][wv * CM_RPT + r], yj);      // rounded product: symmetric in (i, j)
                acc[r] = fma(wk, p, acc[r]);
            }
        }
    }
}

__global__ void __launch_bounds__(256)
cmaes_cov_update_kernel(int N, size_t ld, int mu, int mu_neg, double* __restrict__ C, double* __restrict__ Yneg,
                        double* __restrict__ dC, const double* __restrict__ Ypos, const double* __restrict__ wpos,
                        const double* __restrict__ Vneg, const double* __restrict__ wneg, const double* __restrict__ pc,
                        const double* __restrict__ scal) {
    __shared__ CmTileLds s;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int i0 = blockIdx.y * CM_TI, j0 = blockIdx.x * CM_TJ;
    const int j = j0 + lane;
    const bool col_live = j < N;
    const double s0 = scal[0], s1 = scal[1], s2 = scal[2];

    // both matrices' tile rows are requested before anything waits on them: 16 loads in flight per lane
    double c_old[CM_RPT], y_old[CM_RPT], acc[CM_RPT];
#pragma unroll
    for (int r = 0; r < CM_RPT; ++r) {
        const int i = i0 + wv * CM_RPT + r;
        const bool live = col_live && i < N;
        c_old[r] = live ? C[(size_t)i * ld + j] : 0.0;
        y_old[r] = (live && Yneg != nullptr) ? Yneg[(size_t)i * ld + j] : 0.0;
    }
#pragma unroll
    for (int r = 0; r < CM_RPT; ++r) acc[r] = __dmul_rn(s0, c_old[r]);
    cm_accumulate(s, Ypos, wpos, mu, N, i0, j0, tid, wv, lane, acc);
    // the rank-one term, last
    const double pcj = col_live ? pc[j] : 0.0;
#pragma unroll
    for (int r = 0; r < CM_RPT; ++r) {
        const int i = i0 + wv * CM_RPT + r;
        if (col_live && i < N) {
            const double v = fma(s1, __dmul_rn(pc[i], pcj), acc[r]);
            C[(size_t)i * ld + j] = v;
            if (i == j) dC[i] = v;
        }
    }
    if (Yneg == nullptr) return;                           // CMA_active off (uniform over the grid)

#pragma unroll
    for (int r = 0; r < CM_RPT; ++r) acc[r] = __dmul_rn(s2, y_old[r]);
    if (mu_neg > 0) cm_accumulate(s, Vneg, wneg, mu_neg, N, i0, j0, tid, wv, lane, acc);
#pragma unroll
    for (int r = 0; r < CM_RPT; ++r) {
        const int i = i0 + wv * CM_RPT + r;
        if (col_live && i < N) Yneg[(size_t)i * ld + j] = acc[r] - c_old[r];
    }
}

}  // namespace rl

using namespace rl;

extern "C" int rl_cmaes_cov_update(int N, int ld, int mu, int mu_neg, double* C, double* Yneg, double* dC,
                                   const double* Ypos, const double* wpos, const double* Vneg, const double* wneg,
                                   const double* pc, const double* scal, void* stream) {
    if (N <= 0 || ld < N || mu <= 0 || mu_neg < 0 || !C || !dC || !Ypos || !wpos || !pc || !scal)
        return set_error(RL_ERR_ARG, "rl_cmaes_cov_update: bad argument (N > 0, ld >= N, mu > 0, mu_neg >= 0, non-NULL state)");
    if (mu_neg > 0 && (!Yneg || !Vneg || !wneg))
        return set_error(RL_ERR_ARG, "rl_cmaes_cov_update: mu_neg > 0 needs Yneg, Vneg and wneg");
    const int gx = (N + CM_TJ - 1) / CM_TJ, gy = (N + CM_TI - 1) / CM_TI;
    if (gy > 65535)
        return set_error(RL_ERR_UNSUPPORTED, "rl_cmaes_cov_update: N = %d is above %d", N, 65535 * CM_TI);
    hipLaunchKernelGGL(cmaes_cov_update_kernel, dim3(gx, gy), dim3(256), 0, (hipStream_t)stream, N, (size_t)ld, mu, mu_neg,
                       C, Yneg, dC, Ypos, wpos, Vneg, wneg, pc, scal);
    return check_launch("cmaes_cov_update_kernel");
}
