// reps_kernels.hip -- the dual function of REPS (rllab/algos/reps.py:101-102,162-187, features :207-211, feature
// differences :228-238) and its sample weights (:104-112) on dense [T][n] planes, each as ONE read of the batch.
//
//   phi(o, t)   = [clip(o, -10, 10), clip(o, -10, 10)^2, al, al^2, al^3, 1],  al = t / 100        (d = 2 Do + 4)
//   fd_b        = phi(next sample of the same path) - phi_b      (zero vector after a path's last sample)
//   delta_b     = r_b + fd_b . v
//   z_b         = delta_b / eta,   m = max_b z_b
//   rl_reps_dual    -> [ m, S = sum exp(z - m), S_delta = sum exp(z - m) delta, count, S_phi[d] = sum exp(z - m) fd ]
//   rl_reps_weights -> w_b = exp(z_b - m)   (0 on invalid samples)
//
// The feature matrix (d x B doubles, 0.7 GB at 500 x 4096 x 20) is never built.  A lane owns one env column and walks a
// chunk of time steps with one row of look-ahead in registers, so that every observation is read once (plus one row per
// chunk) and every wavefront load is 256 contiguous bytes.  All arithmetic on the samples is float64: with eta = 1e-2 a
// float32 delta of magnitude 1e3 would move z by 1e-2.
//
// One pass, no second read for the maximum: a lane accumulates against a REFERENCE exponent `ref` (a z it has seen) and
// rescales its sums only when a new z exceeds it by more than RESCALE_GAP -- in float64 exp(RESCALE_GAP) is far from
// overflow, so the rescale (d + 2 multiplications) is rare instead of once per new maximum.  The true maximum is tracked
// separately; the workgroup's partial row is expressed against its own maximum, and reps_reduce_kernel folds the rows
// against the batch maximum in a FIXED order (strided segments, then a tree), so two launches on the same input are
// bit-identical.
#include <hip/hip_runtime.h>
#include <math.h>
#include "../../include/rllab_amd.h"
#include "capi_util.h"

namespace rl {

constexpr int RP_MAX_DO = 30;          // 2 Do + 4 <= 64
constexpr int RP_MAX_D = 64;
constexpr int RP_HEAD = 4;             // m, S, S_delta, count
constexpr int RP_ROW = RP_HEAD + RP_MAX_D;      // doubles per partial row
constexpr int RP_WAVES = 4;            // time chunks per workgroup (one wavefront each)
constexpr int RP_MAX_PART = 1024;      // partial rows reps_reduce_kernel folds
constexpr int RP_SEG = 8;              // strided segments of the fold
constexpr int RP_RED_THREADS = 576;    // reps_reduce_kernel: RP_ROW x RP_SEG = 544 summing threads, whole wavefronts
constexpr double RESCALE_GAP = 50.0;

struct RepsV { double v[RP_MAX_D]; };  // by value in the kernel arguments: no upload per evaluation

struct RepsPlan { int col_groups, chunks, L, grid_y; };

// time steps per wavefront: about 2048 wavefronts (two per SIMD) when the batch is large enough, at least 8 steps so
// that the look-ahead row and the wavefront's final reduction stay a small part of its work
static RepsPlan reps_plan(int T, int n) {
    RepsPlan p;
    p.col_groups = (n + 63) / 64;
    int want = (2048 + p.col_groups - 1) / p.col_groups;
    int L = (T + want - 1) / want;
    if (L < 8) L = 8;
    if (L > T) L = T;
    for (;;) {
        p.L = L;
        p.chunks = (T + L - 1) / L;
        p.grid_y = (p.chunks + RP_WAVES - 1) / RP_WAVES;
        if ((size_t)p.col_groups * p.grid_y <= (size_t)RP_MAX_PART || L >= T) break;
        L *= 2;
        if (L > T) L = T;
    }
    return p;
}

// one row of one column: clipped observations (float32 values, exact) and phi . v in float64
template <int DOP>
__device__ __forceinline__ double reps_row(int Do, const float* __restrict__ obs, size_t plane, size_t off, int tin,
                                           const RepsV& pv, float (&c)[DOP]) {
    double acc = 0.0;
#pragma unroll
    for (int d = 0; d < DOP; ++d) {
        c[d] = 0.0f;
        if (d < Do) {
            const float o = fminf(fmaxf(obs[(size_t)d * plane + off], -10.0f), 10.0f);
            c[d] = o;
            const double od = (double)o;
            acc += pv.v[d] * od;
            acc += pv.v[Do + d] * (od * od);
        }
    }
    const double al = (double)tin / 100.0;
    acc += pv.v[2 * Do] * al;
    acc += pv.v[2 * Do + 1] * (al * al);
    acc += pv.v[2 * Do + 2] * (al * al * al);
    acc += pv.v[2 * Do + 3];
    return acc;
}

__device__ __forceinline__ double wave_sum(double x) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) x += __shfl_xor(x, s, 64);
    return x;
}

__device__ __forceinline__ double wave_max(double x) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) x = fmax(x, __shfl_xor(x, s, 64));
    return x;
}

// WEIGHTS = false: partial row of the workgroup.  WEIGHTS = true: w[t][n] against the batch maximum *m_dev.
template <int DOP, bool WEIGHTS>
__global__ void __launch_bounds__(64 * RP_WAVES)
reps_kernel(int T, int n, int Do, int L, const float* __restrict__ obs, const float* __restrict__ rewards,
            const int32_t* __restrict__ tin, const uint8_t* __restrict__ dones, const uint8_t* __restrict__ valid,
            double eta, RepsV pv, const double* __restrict__ m_dev, float* __restrict__ w_out,
            double* __restrict__ part) {
    constexpr int NA = 2 * DOP + 4;
    __shared__ double s_red[RP_WAVES][RP_ROW];
    const int lane = threadIdx.x, wv = threadIdx.y;
    const int col = blockIdx.x * 64 + lane;
    const bool live = col < n;
    const int cc = live ? col : n - 1;            // dead lanes read a valid address and count nothing
    const int t0 = (blockIdx.y * RP_WAVES + wv) * L;
    const int t1 = min(T, t0 + L);
    const size_t plane = (size_t)T * n;

    double A[NA];
#pragma unroll
    for (int k = 0; k < NA; ++k) A[k] = 0.0;
    double S = 0.0, Sd = 0.0, cnt = 0.0;
    double ref = -INFINITY, zmax = -INFINITY;
    const double m_all = WEIGHTS ? m_dev[0] : 0.0;

    if (t0 < t1) {
        float cur[DOP], nxt[DOP];
#pragma unroll
        for (int d = 0; d < DOP; ++d) nxt[d] = 0.0f;
        size_t off = (size_t)t0 * n + cc;
        int tin_c = tin[off];
        bool val_c = live && valid[off] != 0;
        double pv_c = reps_row<DOP>(Do, obs, plane, off, tin_c, pv, cur);
        for (int t = t0; t < t1; ++t) {
            const bool has_row = t + 1 < T;                    // wave-uniform
            int tin_n = 0;
            bool val_n = false;
            double pv_n = 0.0;
            if (has_row) {
                tin_n = tin[off + n];
                val_n = live && valid[off + n] != 0;
                pv_n = reps_row<DOP>(Do, obs, plane, off + n, tin_n, pv, nxt);
            }
            const bool link = has_row && val_n && dones[off] == 0;
            const double r = (double)rewards[off];
            const double delta = r + (link ? pv_n : 0.0) - pv_c;
            const double z = delta / eta;
            if (WEIGHTS) {
                if (live) w_out[off] = val_c ? (float)exp(z - m_all) : 0.0f;
            } else if (val_c) {
                zmax = fmax(zmax, z);
                if (z - ref > RESCALE_GAP) {                   // also the first valid sample (ref = -inf)
                    const double f = exp(ref - z);
                    S *= f;
                    Sd *= f;
#pragma unroll
                    for (int k = 0; k < NA; ++k) A[k] *= f;
                    ref = z;
                }
                const double e = exp(z - ref);
                S += e;
                Sd += e * delta;
                cnt += 1.0;
                const double ln = link ? 1.0 : 0.0;
#pragma unroll
                for (int d = 0; d < DOP; ++d) {
                    if (d < Do) {
                        const double a = (double)cur[d], b = link ? (double)nxt[d] : 0.0;
                        A[d] += e * (b - a);
                        A[DOP + d] += e * (b * b - a * a);
                    }
                }
                const double al_c = (double)tin_c / 100.0, al_n = ln * ((double)tin_n / 100.0);
                A[2 * DOP] += e * (al_n - al_c);
                A[2 * DOP + 1] += e * (al_n * al_n - al_c * al_c);
                A[2 * DOP + 2] += e * (al_n * al_n * al_n - al_c * al_c * al_c);
                A[2 * DOP + 3] += e * (ln - 1.0);
            }
            // the look-ahead row becomes the current one
#pragma unroll
            for (int d = 0; d < DOP; ++d) cur[d] = has_row ? nxt[d] : 0.0f;
            pv_c = pv_n;
            tin_c = tin_n;
            val_c = val_n;
            off += n;
        }
    }
    if (WEIGHTS) return;

    // workgroup partial row, expressed against the workgroup's own maximum
    const double wmax = wave_max(zmax);
    if (lane == 0) s_red[wv][0] = wmax;
    __syncthreads();
    double gmax = s_red[0][0];
#pragma unroll
    for (int w = 1; w < RP_WAVES; ++w) gmax = fmax(gmax, s_red[w][0]);
    __syncthreads();
    const double f = (ref == -INFINITY) ? 0.0 : exp(ref - gmax);      // ref <= zmax <= gmax: never above 1
    const double s1 = wave_sum(S * f), s2 = wave_sum(Sd * f), s3 = wave_sum(cnt);
    if (lane == 0) { s_red[wv][1] = s1; s_red[wv][2] = s2; s_red[wv][3] = s3; }
    // A is laid out [DOP | DOP | 4]; the row wants the reference order [Do | Do | 4]
#pragma unroll
    for (int d = 0; d < DOP; ++d) {
        if (d < Do) {
            const double a = wave_sum(A[d] * f), b = wave_sum(A[DOP + d] * f);
            if (lane == 0) { s_red[wv][RP_HEAD + d] = a; s_red[wv][RP_HEAD + Do + d] = b; }
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double a = wave_sum(A[2 * DOP + k] * f);
        if (lane == 0) s_red[wv][RP_HEAD + 2 * Do + k] = a;
    }
    __syncthreads();
    const int tid = wv * 64 + lane;
    const int width = RP_HEAD + 2 * Do + 4;
    if (tid < width) {
        double* row = part + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * RP_ROW;
        double x = gmax;
        if (tid > 0) {
            x = s_red[0][tid];
#pragma unroll
            for (int w = 1; w < RP_WAVES; ++w) x += s_red[w][tid];
        }
        row[tid] = x;
    }
}

// out[0] = max_p m_p;  out[k] = sum_p row_p[k] exp(m_p - out[0])  (count: plain sum), in a fixed order: RP_SEG strided
// partial sums per entry, then their tree.  One workgroup.
__global__ void __launch_bounds__(RP_RED_THREADS)
reps_reduce_kernel(const double* __restrict__ part, int P, int width, double* __restrict__ out) {
    __shared__ double s_f[RP_MAX_PART];
    __shared__ double s_max[RP_RED_THREADS / 64];
    __shared__ double s_sum[RP_SEG][RP_ROW];
    const int tid = threadIdx.x;
    double mx = -INFINITY;
    for (int p = tid; p < P; p += blockDim.x) mx = fmax(mx, part[(size_t)p * RP_ROW]);
    mx = wave_max(mx);
    if ((tid & 63) == 0) s_max[tid >> 6] = mx;
    __syncthreads();
    double m = s_max[0];
    for (int w = 1; w < RP_RED_THREADS / 64; ++w) m = fmax(m, s_max[w]);
    for (int p = tid; p < P; p += blockDim.x) {
        const double mp = part[(size_t)p * RP_ROW];
        s_f[p] = (mp == -INFINITY) ? 0.0 : exp(mp - m);
    }
    __syncthreads();
    const int k = tid % RP_ROW, seg = tid / RP_ROW;           // seg == RP_SEG: the spare threads of the last wavefront
    double acc = 0.0;
    if (seg < RP_SEG && k >= 1 && k < width)
        for (int p = seg; p < P; p += RP_SEG) acc += part[(size_t)p * RP_ROW + k] * (k == 3 ? 1.0 : s_f[p]);
    if (seg < RP_SEG) s_sum[seg][k] = acc;
    __syncthreads();
    for (int half = RP_SEG / 2; half >= 1; half >>= 1) {
        if (seg < half) s_sum[seg][k] += s_sum[seg + half][k];
        __syncthreads();
    }
    if (seg == 0 && k < width) out[k] = (k == 0) ? m : s_sum[0][k];
}

template <bool WEIGHTS>
static void reps_launch(int T, int n, int Do, const RepsPlan& p, const float* obs, const float* rewards, const int32_t* tin,
                        const uint8_t* dones, const uint8_t* valid, double eta, const RepsV& pv, const double* m_dev,
                        float* w_out, double* part, hipStream_t stream) {
    const dim3 grid(p.col_groups, p.grid_y), block(64, RP_WAVES);
#define RL_REPS_LAUNCH(DOP)                                                                                              \
    hipLaunchKernelGGL((reps_kernel<DOP, WEIGHTS>), grid, block, 0, stream, T, n, Do, p.L, obs, rewards, tin, dones,     \
                       valid, eta, pv, m_dev, w_out, part)
    // the observation loop is unrolled to one of five widths (the accumulators live in registers); rows beyond Do are
    // skipped by a wave-uniform test
    if (Do <= 4) RL_REPS_LAUNCH(4);
    else if (Do <= 8) RL_REPS_LAUNCH(8);
    else if (Do <= 13) RL_REPS_LAUNCH(13);
    else if (Do <= 21) RL_REPS_LAUNCH(21);
    else RL_REPS_LAUNCH(30);
#undef RL_REPS_LAUNCH
}

static int reps_check(const char* who, int T, int n, int obs_dim, const void* obs, const void* rewards, const void* tin,
                      const void* dones, const void* valid, double eta, const double* v) {
    if (T <= 0 || n <= 0 || obs_dim <= 0 || obs_dim > RP_MAX_DO || !obs || !rewards || !tin || !dones || !valid || !v ||
        !(eta > 0.0) || !isfinite(eta))
        return set_error(RL_ERR_ARG, "%s: bad argument (0 < obs_dim <= %d, eta > 0)", who, RP_MAX_DO);
    return 0;
}

}  // namespace rl

using namespace rl;

extern "C" size_t rl_reps_workspace_bytes(int T, int n) {
    if (T <= 0 || n <= 0) return 0;
    const RepsPlan p = reps_plan(T, n);
    return (size_t)p.col_groups * p.grid_y * RP_ROW * sizeof(double);
}

extern "C" int rl_reps_dual(int T, int n, int obs_dim, const float* obs, const float* rewards, const int32_t* tin,
                            const uint8_t* dones, const uint8_t* valid, double eta, const double* v_host,
                            void* workspace, size_t workspace_bytes, double* out, void* stream) {
    if (int rc = reps_check("rl_reps_dual", T, n, obs_dim, obs, rewards, tin, dones, valid, eta, v_host)) return rc;
    if (!workspace || !out) return set_error(RL_ERR_ARG, "rl_reps_dual: bad argument");
    const RepsPlan p = reps_plan(T, n);
    const size_t P = (size_t)p.col_groups * p.grid_y;
    if (P > (size_t)RP_MAX_PART)
        return set_error(RL_ERR_UNSUPPORTED, "rl_reps_dual: more than %d x 64 env columns", RP_MAX_PART);
    if (workspace_bytes < P * RP_ROW * sizeof(double)) return set_error(RL_ERR_ARG, "rl_reps_dual: workspace too small");
    RepsV pv;
    const int d = 2 * obs_dim + 4;
    for (int k = 0; k < RP_MAX_D; ++k) pv.v[k] = k < d ? v_host[k] : 0.0;
    reps_launch<false>(T, n, obs_dim, p, obs, rewards, tin, dones, valid, eta, pv, nullptr, nullptr, (double*)workspace,
                       (hipStream_t)stream);
    hipLaunchKernelGGL(reps_reduce_kernel, dim3(1), dim3(RP_RED_THREADS), 0, (hipStream_t)stream,
                       (const double*)workspace, (int)P, RP_HEAD + d, out);
    return check_launch("reps_kernel");
}

extern "C" int rl_reps_weights(int T, int n, int obs_dim, const float* obs, const float* rewards, const int32_t* tin,
                               const uint8_t* dones, const uint8_t* valid, double eta, const double* v_host,
                               const double* dual_out, float* weights, void* stream) {
    if (int rc = reps_check("rl_reps_weights", T, n, obs_dim, obs, rewards, tin, dones, valid, eta, v_host)) return rc;
    if (!dual_out || !weights) return set_error(RL_ERR_ARG, "rl_reps_weights: bad argument");
    const RepsPlan p = reps_plan(T, n);
    RepsV pv;
    const int d = 2 * obs_dim + 4;
    for (int k = 0; k < RP_MAX_D; ++k) pv.v[k] = k < d ? v_host[k] : 0.0;
    reps_launch<true>(T, n, obs_dim, p, obs, rewards, tin, dones, valid, eta, pv, dual_out, weights, nullptr,
                      (hipStream_t)stream);
    return check_launch("reps_kernel");
}
