// fvp_split_common.h -- what the split-operand Fisher-vector products share: policy_split_kernels.hip (three-way bf16),
// policy_splith_kernels.hip (two-way f16), policy_split16_kernels.hip (16-sample tiles) and policy_csplit_kernels.hip
// (cooperative).  The entry points the files call across each other and policy_kernels.hip calls, the (obs_dim, act_dim)
// lists the kernels are instantiated for, the host side of a launch, and the device code that is the same in every file and
// whose move here leaves every kernel's instruction stream as it was: the small f32 helpers, the log-std Fisher coefficient and
// the fold of a workgroup's wavefronts into one partial row.  The split arithmetic itself (Parts / PB / PA, the cross-term
// products, the transposes, the tile loops) stays per file -- and so, for now, do the output layer's thin products, the
// back-propagation through it and the per-lane reductions in front of the fold, copies though they are: as inline functions
// they reach the optimiser in another order and every kernel comes out with other registers and another schedule.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/rllab_amd.h"
#include "capi_util.h"
#include "policy_mfma.h"

namespace rl {

// ---- across translation units ---------------------------------------------------------------------------------------------
int launch_reduce_rows(const float* partial, int rows, int cols, double* out, hipStream_t st);   // policy_kernels.hip
bool net_has_narrow_kernel(int obs_dim, int act_dim, int h0, int h1, int h2);                    // policy_kernels.hip
// <x>_fvp_takes: would rl_policy_fvp of this batch run on that file's kernels (host only, launches nothing);
// <x>_fvp_dispatch: launch it there, or RL_SPLIT_NOT_TAKEN.  The order in which rl_policy_fvp asks: FVP_KERNELS, policy_kernels.hip
bool split_fvp_takes(const rl_policy_batch* g);
bool split16_fvp_takes(const rl_policy_batch* g);
bool splith_fvp_takes(const rl_policy_batch* g);
bool csplit_fvp_takes(const rl_policy_batch* g);
int split_fvp_dispatch(const rl_policy_batch* g, const float* vec, void* ws, size_t ws_bytes, double* out, hipStream_t st);
int split16_fvp_dispatch(const rl_policy_batch* g, const float* vec, void* ws, size_t ws_bytes, double* out, hipStream_t st);
int splith_fvp_dispatch(const rl_policy_batch* g, const float* vec, void* ws, size_t ws_bytes, double* out, hipStream_t st);
int csplit_fvp_dispatch(const rl_policy_batch* g, const float* vec, void* ws, size_t ws_bytes, double* out, hipStream_t st);
size_t csplit_workspace_bytes_for(int obs_dim, int act_dim, int h0, int h1, int h2);             // 0 = not its shape

// ---- (obs_dim, act_dim) lists ------------------------------------------------------------------------------------------------
// fvp_split_kernel / fvp_splith_kernel, (32, 32): the HIP-native envs (a (32, 32) net is rllab's default policy for every one
// of them) + the one-output net on the Swimmer's observations.  Heads wider than two outputs run one wavefront per SIMD:
// their per-lane sums of the thin products (16 x act_dim registers) do not fit beside 256.
#define SPLIT_SHAPES(X) X(4, 1) X(6, 1) X(11, 1) X(13, 2) X(13, 1) X(20, 3) X(20, 6) X(21, 6)
// fvp_split64_kernel / fvp_splith64_kernel, (64, 64): the pairs policy_pass_kernel<Net<.., 64>> caches activations for
#define SPLIT64_SHAPES(X) X(4, 1) X(6, 1) X(11, 1) X(13, 2) X(20, 3) X(20, 6) X(21, 6)
// fvp_split16_kernel, (32, 32): at most two actions (the per-lane sums of the output layer's outer product are 8 act_dim
// registers of the 128)
#define SPLIT16_SHAPES(X) X(4, 1) X(6, 1) X(11, 1) X(13, 2) X(13, 1)
// (obs_dim, act_dim, H) of the one-wavefront-per-tile update kernels (two equal tanh layers): every HIP-native env's pair at 32
// and 64 units (RL_PLANE_NETS: what rl_mlp_forward / rl_mlp_backward are built for) + the one-output value nets.  Everything
// else runs on the cooperative kernels -- and the two families cache their activations in different layouts, which is what
// the split Fisher-vector products ask net_has_narrow_kernel for.
#define RL_PLANE_NETS(X) \
    X(4, 1, 32) X(6, 1, 32) X(11, 1, 32) X(13, 2, 32) X(20, 3, 32) X(20, 6, 32) X(21, 6, 32) \
    X(4, 1, 64) X(6, 1, 64) X(11, 1, 64) X(13, 2, 64) X(20, 3, 64) X(20, 6, 64) X(21, 6, 64)
#define RL_NARROW_NETS(X) RL_PLANE_NETS(X) X(13, 1, 32) X(20, 1, 32) X(21, 1, 32)

// ---- host: one launch -----------------------------------------------------------------------------------------------------
// the fields every one-wavefront-per-tile kernel's Args has (its own struct: the kernels' symbols and argument offsets are part
// of the pinned instruction streams); `partial` is set by launch_tiles
template <class A>
static A make_args(const rl_policy_batch* g, const float* vec) {
    A a = {};
    a.B = g->n_samples; a.theta = g->theta; a.vec = vec; a.acts = g->activations; a.obs = g->obs; a.weight = g->weights;
    a.inv_count = g->inv_count; a.log_min_std = g->log_min_std;
    return a;
}
// `grid` workgroups of Kern write one partial row of P floats each at a.partial; their float64 column sums are `out`
template <auto Kern, class A>
static int launch_partial_rows(const char* name, const A& a, int grid, int block, int lds_limit, int lds_bytes, int P, double* out,
                               hipStream_t st) {
    static bool attr_set = false;      // per process and kernel instantiation, not per device (allow_dynamic_lds)
    if (int rc = allow_dynamic_lds(Kern, lds_limit, attr_set)) return rc;
    hipLaunchKernelGGL(Kern, dim3(grid), dim3(block), lds_bytes, st, a);
    if (int rc = check_launch(name)) return rc;
    return launch_reduce_rows(a.partial, grid, P, out, st);
}
// a kernel whose WAVES wavefronts per workgroup each own tiles of TILE samples: one workgroup per CU, partial rows in `ws`
template <auto Kern, int WAVES, int TILE, int LDS_BYTES, int P, class A>
static int launch_tiles(const char* name, A a, void* ws, size_t ws_bytes, double* out, hipStream_t st) {
    const int n_tiles = a.B / TILE;
    int grid = (n_tiles + WAVES - 1) / WAVES;
    if (grid > 256) grid = 256;
    const size_t need = (size_t)grid * P * sizeof(float);
    if (ws_bytes < need) return set_error(RL_ERR_ARG, "policy pass workspace too small: %zu < %zu bytes", ws_bytes, need);
    a.partial = (float*)ws;
    return launch_partial_rows<Kern>(name, a, grid, WAVES * WV, LDS_BYTES, LDS_BYTES, P, out, st);
}

// ---- device: the f32 part -----------------------------------------------------------------------------------------------------
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(4))) float f32x4;

// value + the value of the same sample in the other lane half, without an LDS round trip (v_permlane32_swap)
__device__ __forceinline__ float half_sum_swap(float v) {
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
// registers (2 j, 2 j + 1) of a fragment as one packed value
__device__ __forceinline__ f32x2 pair_of(const f32x16& v, int j) { return f32x2{v[2 * j], v[2 * j + 1]}; }
__device__ __forceinline__ void set_pair(f32x16& v, int j, f32x2 p) { v[2 * j] = p[0]; v[2 * j + 1] = p[1]; }

// log_std block of the Fisher: d2KL/ds2 = 4 v (2 v - eps) / (2 v + eps)^2, v = sigma^2; 0 where min_std holds log_std
__device__ __forceinline__ float log_std_fisher(float vv, bool floored) {
    const float e = 1e-8f;
    return floored ? 0.0f : 4.0f * vv * (2.0f * vv - e) / ((2.0f * vv + e) * (2.0f * vv + e));
}

// Every wavefront has laid its contribution out as one row of P floats at the start of LDS (each parameter has exactly one
// contributor per wavefront): the columns are summed in wavefront order -- the same sums as folding the wavefronts one after
// the other, with two workgroup barriers instead of WAVES + 2 -- into this workgroup's partial row.
template <int WAVES, int P>
__device__ __forceinline__ void fold_rows(const char* smem, float* partial) {
    float* row = partial + (size_t)blockIdx.x * P;
    for (int k = threadIdx.x; k < P; k += WAVES * WV) {
        float t = 0.0f;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) t += reinterpret_cast<const float*>(smem)[w * P + k];
        row[k] = t;
    }
}

}  // namespace rl
