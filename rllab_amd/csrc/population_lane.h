// population_lane.h -- what the kernels with one parameter vector per env share (population_kernels.hip,
// population_gru_kernels.hip): how a lane reads ITS candidate out of the transposed population image, and the returns of
// its env's first path.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "rollout_lane.h"

namespace rl {

// Rows of theta_pop_T read one after the other: the row address is a scalar that walks (one s_add_u32 / s_addc_u32 pair
// per row), the load is the scalar-base + 32-bit lane offset form of global_load -- the reading twin of store_planes
// (rollout_lane.h), for the same reason: P hoisted 64-bit row addresses fit no register file.
struct RowWalk {
    uintptr_t walk;
    __device__ __forceinline__ RowWalk(const float* theta_T, size_t row_bytes, int row)
        : walk(reinterpret_cast<uintptr_t>(theta_T) + (size_t)row * row_bytes) {}
    __device__ __forceinline__ float next(size_t row_bytes, uint32_t& lane_bytes) {
        typedef const __attribute__((address_space(1))) float* global_ptr;
        asm volatile("" : "+s"(walk));
        asm volatile("" : "+v"(lane_bytes));
        const float v = *reinterpret_cast<global_ptr>(walk + lane_bytes);
        walk += row_bytes;
        return v;
    }
    __device__ __forceinline__ void skip(size_t bytes) { walk += bytes; }    // (wraps for a step back: unsigned arithmetic)
};

// the first path of this lane's env (cem.py:46-56: one rollout per candidate, its discounted and undiscounted return):
// float32 sums over the rewards as recorded, up to the first done
struct FirstPath {
    float ret_disc = 0.0f, ret_undisc = 0.0f;
    double gpow = 1.0;                        // discount^t: float64, so the only float32 roundings are the sum's
    int first_len = 0;
    bool first_open = true;
    __device__ __forceinline__ void stepped(float rs, bool d, double discount) {
        if (first_open) {
            ret_disc = __builtin_fmaf((float)gpow, rs, ret_disc);
            ret_undisc += rs;
            gpow *= discount;
            first_len += 1;
            first_open = !d;
        }
    }
    __device__ __forceinline__ void store(float* first_path, int n, int i) const {      // first_path [3][n]
        const float fp[3] = {ret_disc, ret_undisc, (float)first_len};
        uint32_t lane_f32 = (uint32_t)i * 4;
        store_planes<3>(first_path, (size_t)n, lane_f32, fp);
    }
};

}  // namespace rl
