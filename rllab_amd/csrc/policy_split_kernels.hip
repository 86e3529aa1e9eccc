// policy_split_kernels.hip -- the Fisher-vector product of a (32, 32) tanh GaussianMLPPolicy on the bf16 matrix
// pipe at f32 accuracy: every f32 operand is split three ways, x = hi + mid + lo with each part a bf16 (exact: the
// parts are successive round-to-nearest residuals), and a product of two operands is the sum of the six cross terms
// hi hi + hi mid + mid hi + hi lo + lo hi + mid mid on v_mfma_f32_32x32x16_bf16 with f32 accumulation.  The dropped
// terms (mid lo + lo mid + lo lo) are at most 2^-23 of |a b| -- two f32 roundings -- when every part sits at its bound, 2^-28
// in the mean and of either sign (tests/test_split_arithmetic.py); measured on the device against float64 the six-term
// dot product is three times closer than an f32 fma chain (tools/ubench/bf16_split_layout.hip).
//
// Why: v_mfma_f32_32x32x2_f32 runs at the f32 VECTOR rate and shares the vector datapath (policy_kernels.hip's
// product retires a 32-sample tile in 7.9 k cycles against a floor of 5.06 k matrix + 1.4 k vector cycles,
// profiles/r03_notes.md); the bf16 pipe is 16 times faster and runs beside the vector ALU, so the six terms cost
// 6/16 of the f32 matrix cycles and the tile becomes vector-bound (the splits).
//
// What it computes: rl_policy_fvp on cached activations (rllab/optimizers/conjugate_gradient_optimizer.py:27-55 at
// theta_new == theta_old, see policy_kernels.hip's header) -- same inputs, same partial-row / float64 row reduction,
// a result that differs from policy_pass_kernel<N, MODE_FVP, true> by rounding only.
//
// Mapping.  A wavefront owns tiles of 32 samples.  All f32 fragments are "sample-major": lane (s = lane & 31,
// half = lane >> 5) holds sample s and the 16 units frag_unit(r, half) -- the layout the matrix pipe produces and the
// layout the gradient pass left the activations in; a fragment's split parts are directly the B operand of the next
// layer (k-block kb = registers 8 kb .. 8 kb + 7).  The products whose contraction runs over SAMPLES (gW1 += h0^T gz1,
// gW0 += x^T gz0) need their operands unit-major: a part is transposed ON THE MATRIX PIPE, part (as the A operand:
// rows = samples) x identity = the same numbers with lane = unit, register = sample, exactly (every output is one
// product with 1), and eight conversions per part pack them back to bf16.  No LDS round trip, no cross-lane
// instruction; the matrix pipe has the slack (24 % busy before, 32 % with the 21 transposition products per tile).
// The thin products of the output layer accumulate per lane and are reduced over the lanes once per launch.
// Two wavefronts per SIMD (eight per workgroup, one workgroup per CU): the stages of a tile are one dependency chain
// (split -> product -> element-wise -> split ...), so the second wavefront is what fills the first one's waits.  With
// 256 registers each the loop-invariant operands (the split fragments of dW0^T, dW1^T, W1^T, W1 and the output layer's
// rows) are staged in LDS once per workgroup and read per use.
#include <hip/hip_runtime.h>
#include <cstdlib>
#include "fvp_split_common.h"

namespace rl {

namespace split {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((address_space(1))) const void* gptr_t;
typedef __attribute__((address_space(3))) void* lptr_t;

constexpr int H = 32;
constexpr int LAND_BYTES = 2 * H * TS * 4;     // h0 | h1 fragments of one tile, as the gradient pass stored them
// LDS image of the loop-invariant operands (two wavefronts per SIMD): KB0 + 6 operand blocks (A1[KB0], A2[2], A3[2],
// A4[2]) x 3 parts x 64 lanes x 16 B, then the output layer per lane half: [half][W2 column k: 16 rows | dW2 ... | db1 16]
constexpr int ops_count(int kb0) { return kb0 + 6; }          // dW0^T: one block per 16 inputs; dW1^T, W1^T, W1: two each
constexpr int ops_bytes(int kb0) { return ops_count(kb0) * 3 * WV * 16; }

struct Args {
    int B;
    const float* theta;
    const float* vec;
    const float* acts;
    const float* obs;
    const float* weight;
    float inv_count;
    float log_min_std;
    float* partial;            // [grid][P]
};

struct Parts { bf16x8 p[3]; };                 // hi, mid, lo of eight values

// Timing ablations (WRONG results, the rest of the instruction stream unchanged; tools/exp/r05_split_ablations.sh):
//   RL_ABL_MFMA   no matrix instructions (operands and accumulator stay live through an empty asm)
//   RL_ABL_SPLIT  no split arithmetic (the parts are left undefined)
//   RL_ABL_FETCH  no per-tile global loads (the first tile's inputs are reused)
//   RL_ABL_OPS    the loop-invariant operands are not re-read from LDS per use
#ifndef RL_ABL_MFMA
#define RL_ABL_MFMA 0
#endif
#ifndef RL_ABL_SPLIT
#define RL_ABL_SPLIT 0
#endif
#ifndef RL_ABL_FETCH
#define RL_ABL_FETCH 0
#endif
#ifndef RL_ABL_OPS
#define RL_ABL_OPS 0
#endif
//   RL_ABL_HALF   two parts per operand and three cross terms per product (the instruction stream a two-way f16 split
//                 would have: timing only)
#ifndef RL_ABL_HALF
#define RL_ABL_HALF 0
#endif
__device__ __forceinline__ f32x16 mfma16(bf16x8 a, bf16x8 b, f32x16 c) {
#if RL_ABL_MFMA
    asm volatile("" : "+v"(c) : "v"(a), "v"(b));
    return c;
#else
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
#endif
}
// c += A B to f32 accuracy: the six cross terms, smallest first
__device__ __forceinline__ f32x16 mm6(const Parts& A, const Parts& B, f32x16 c) {
#if !RL_ABL_HALF
    c = mfma16(A.p[1], B.p[1], c);
    c = mfma16(A.p[0], B.p[2], c);
    c = mfma16(A.p[2], B.p[0], c);
#endif
    c = mfma16(A.p[0], B.p[1], c);
    c = mfma16(A.p[1], B.p[0], c);
    c = mfma16(A.p[0], B.p[0], c);
    return c;
}

// Settled experiments of rounds 5 and 6, once build-time switches of this file; what stayed is the code below, what lost is gone:
//   RL_SPLIT_DOT2 (kept)  the residual  a - bf16(a)  of a pair as two v_dot2c_f32_bf16 (packed rounding x (-1, 0) / (0, -1),
//                  accumulated onto a): every term is exactly representable, so the dot product is the same number
//                  (tools/ubench/dot2_residual.hip checks it bit for bit on the device, denormal residuals included).  The
//                  alternative was two unpack instructions + one packed subtraction (profiles/r05_notes.md section 1.2).
//   RL_SPLIT_PK (kept)  the element-wise stages (tanh derivatives, the output layer's thin products, bias sums) on packed f32
//                  instructions, two values per issue slot; the alternative was one plain instruction per value (same section).
//   RL_SPLIT_SCALAR_SUB (dropped)  without the dot form, the residual as two plain v_sub_f32 instead of one v_pk_add_f32, because
//                  packed f32 instructions of one wavefront do not overlap the matrix instructions of another
//                  (tools/ubench/mfma_bf16_valu_overlap.hip, profiles/r03_notes.md); tools/exp/r05_split_variants.sh timed it
//                  against the dot form, which stayed.
//   RL_SPLIT_ASM_DMA (kept)  the LDS-direct loads of the next tile's inputs as inline asm.  Issued through the builtin, the
//                  compiler has to assume that they write ANY LDS address and puts s_waitcnt vmcnt(0) in front of the next
//                  LDS read it cannot tell apart -- the output layer's rows, a third of the way into the tile: the wavefront
//                  then sits out the rest of the HBM round trip it had meant to hide (timing ablation RL_ABL_FETCH: 19 % of
//                  the kernel).  The asm form is invisible to that pass; the loop's own s_waitcnt vmcnt(0) at the top of the
//                  next tile is the (only) wait the data needs.  The alternative kept observations and weight in registers.
//   RL_SPLIT_BULK_ROWS (kept; round 6)  the output layer's rows of a lane half come in bulk -- per action the 16 rows of W2 and
//                  of its tangent are eight 16-byte LDS reads issued together and waited for once -- and its per-lane dot
//                  products run as FOUR independent packed partial sums.  By the ISA of the round-5 build this stage was one
//                  chain of 16 dependent v_pk_fma_f32 per action (a wait state behind every one) with a ds_read_b128 +
//                  s_waitcnt lgkmcnt(0) in front of every other one: ~20 exposed LDS round trips per tile
//                  (profiles/r06_notes.md section 7; fvp_split64_kernel had this form since round 5).
//   RL_SPLIT_OPS_AHEAD (kept; round 6)  two wavefronts per SIMD, operand blocks in LDS: the three parts of the NEXT operand block
//                  are read before the six products of the current one are issued (and the first block of a chain before
//                  the vector work in front of it); by the ISA every block was read right in front of its use and waited
//                  for -- seven exposed LDS round trips per tile (same section).
//   RL_SPLIT_FILL (dropped; round 6)  vector work that does not depend on a chain of products (the split of dh0, on plain
//                  instructions) issued INSIDE the chain dW1^T h0, in the ~5 issue slots a v_mfma_f32_32x32x16_bf16 leaves its
//                  own wavefront.  MEASURED: nothing (0.2117 - 0.2149 ms with the filler on dot / packed or on plain
//                  instructions against 0.2095 - 0.2147 without, same box, profiles/r06_notes.md section 7) and 17 spilled
//                  registers.
// a - h for a pair a and its packed bf16 rounding h (exact)
// The two selectors (-1, 0) and (0, -1) travel in REGISTERS: handed to the instruction as a constant, (-1, 0) is encoded as
// the inline constant "-1.0", which the VOP2 form of v_dot2c_f32_bf16 reads as the f32 pattern 0xbf800000 = (0, -1) --
// measured on the device (tools/ubench/dot2_residual.hip, first build: every low component wrong); an asm-opaque
// register operand leaves the assembler nothing to encode.
// (a pure asm: identical instances are merged and hoisted out of the tile loop -- two registers per wavefront)
__device__ __forceinline__ bf16x2 dot2_selector(unsigned bits) {
    unsigned v;
    asm("v_mov_b32 %0, %1" : "=v"(v) : "s"(bits));
    return __builtin_bit_cast(bf16x2, v);
}
__device__ __forceinline__ f32x2 residual(f32x2 a, bf16x2 h) {
    const bf16x2 e0 = dot2_selector(0x0000bf80u), e1 = dot2_selector(0xbf800000u);
    return f32x2{__builtin_amdgcn_fdot2_f32_bf16(h, e0, a[0], false), __builtin_amdgcn_fdot2_f32_bf16(h, e1, a[1], false)};
}
// x = hi + mid + lo, each a bf16: successive round-to-nearest residuals (every subtraction is exact)
__device__ __forceinline__ void split_pair(float a0, float a1, Parts& out, int j) {
#if RL_ABL_SPLIT
    {
        unsigned h, m, q;
        asm volatile("" : "=v"(h), "=v"(m), "=v"(q) : "v"(a0), "v"(a1));
        const bf16x2 hh = __builtin_bit_cast(bf16x2, h), mm = __builtin_bit_cast(bf16x2, m), qq = __builtin_bit_cast(bf16x2, q);
        out.p[0][j] = hh[0]; out.p[0][j + 1] = hh[1];
        out.p[1][j] = mm[0]; out.p[1][j + 1] = mm[1];
        out.p[2][j] = qq[0]; out.p[2][j + 1] = qq[1];
        return;
    }
#endif
    const f32x2 a = {a0, a1};
    const bf16x2 h = __builtin_convertvector(a, bf16x2);
    const f32x2 r = residual(a, h);
#if RL_ABL_HALF
    {
        const bf16x2 m = __builtin_convertvector(r * f32x2{2048.0f, 2048.0f}, bf16x2);
        out.p[0][j] = h[0]; out.p[0][j + 1] = h[1];
        out.p[1][j] = m[0]; out.p[1][j + 1] = m[1];
        out.p[2][j] = m[0]; out.p[2][j + 1] = m[1];
        return;
    }
#endif
    const bf16x2 m = __builtin_convertvector(r, bf16x2);
    const f32x2 l = residual(r, m);
    const bf16x2 q = __builtin_convertvector(l, bf16x2);
    out.p[0][j] = h[0]; out.p[0][j + 1] = h[1];
    out.p[1][j] = m[0]; out.p[1][j + 1] = m[1];
    out.p[2][j] = q[0]; out.p[2][j + 1] = q[1];
}
__device__ __forceinline__ void split8(const float* v, Parts& out) {
#pragma unroll
    for (int j = 0; j < 8; j += 2) split_pair(v[j], v[j + 1], out, j);
}
// a 16-register fragment -> the operands of its two k-blocks (registers 8 kb .. 8 kb + 7)
__device__ __forceinline__ void split_frag(const f32x16& v, Parts (&out)[2]) {
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int j = 0; j < 8; j += 2) split_pair(v[8 * kb + j], v[8 * kb + j + 1], out[kb], j);
}
// an f32 fragment whose values ARE bf16 numbers (a transposed part) -> the operands of its two k-blocks
__device__ __forceinline__ void pack_exact(const f32x16& d, Parts (&out)[2], int p) {
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int j = 0; j < 8; j += 2) {
            const f32x2 a = {d[8 * kb + j], d[8 * kb + j + 1]};
            const bf16x2 h = __builtin_convertvector(a, bf16x2);
            out[kb].p[p][j] = h[0]; out[kb].p[p][j + 1] = h[1];
        }
}
// sample-major parts of a 32-unit fragment -> unit-major parts: lane (unit, half) receives the samples
// frag_unit(8 kb + j, half) as k-block kb.  part (A: rows = samples, k = units) x identity, on the matrix pipe, exact.
__device__ __forceinline__ void transpose_units(const Parts (&f)[2], const bf16x8 (&Id)[2], Parts (&out)[2]) {
#pragma unroll
    for (int p = 0; p < (RL_ABL_HALF ? 2 : 3); ++p) {
        f32x16 d;
#pragma unroll
        for (int r = 0; r < 16; ++r) d[r] = 0.0f;
        d = mfma16(f[0].p[p], Id[0], d);
        d = mfma16(f[1].p[p], Id[1], d);
        pack_exact(d, out, p);
    }
}
// the x fragment (KB0 k-blocks of 16 inputs): lane (input d, half); lanes beyond the inputs receive zeros
template <int KB0>
__device__ __forceinline__ void transpose_inputs(const Parts (&f)[KB0], const bf16x8 (&Idx)[KB0], Parts (&out)[2]) {
#pragma unroll
    for (int p = 0; p < (RL_ABL_HALF ? 2 : 3); ++p) {
        f32x16 d;
#pragma unroll
        for (int r = 0; r < 16; ++r) d[r] = 0.0f;
#pragma unroll
        for (int kb = 0; kb < KB0; ++kb) d = mfma16(f[kb].p[p], Idx[kb], d);
        pack_exact(d, out, p);
    }
}

// out = acc * (1 - h h), element-wise over a fragment (the tanh derivative through the activation itself)
__device__ __forceinline__ void times_dtanh(const f32x16& acc, const f32x16& h, f32x16& out) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const f32x2 hh = pair_of(h, j);
        const f32x2 d = __builtin_elementwise_fma(-hh, hh, f32x2{1.0f, 1.0f});
        set_pair(out, j, pair_of(acc, j) * d);
    }
}

template <int DO, int DA, int WPS>
__global__ void __launch_bounds__(4 * WPS * WV, 1) fvp_split_kernel(Args a) {
    using N = Net<DO, DA, H>;
    constexpr int P = N::P;
    constexpr int WAVES = 4 * WPS;
    constexpr int KB0 = (DO + 1 + 15) / 16;        // k-blocks of the input layer (inputs + the bias slot)
    constexpr int N_OPS = ops_count(KB0), OPS_BYTES = ops_bytes(KB0);
    constexpr bool INV_LDS = (WPS == 2);           // matrix operands in LDS (256 registers per wavefront)
    constexpr bool TAIL_LDS = INV_LDS || DA > 2;   // the output layer's rows in LDS (wide heads: 32 DA registers otherwise)
    constexpr int TAILV = 16 * DA * 2 + 16;        // floats per lane half: W2 rows | dW2 rows | db1
    constexpr int SPILL_BYTES = INV_LDS ? 2 * 3 * WV * 16 : 0;   // a wavefront's h0 parts wait here for the back-propagation
    // the next tile's observations + weight land as XPIECES pieces of 8 rows x 32 samples (rows < DO: inputs, row DO: the
    // weight -- its slot in x_ext is the constant 1): an LDS-direct piece costs the CU ~120 - 150 cycles whatever it carries
    // (profiles/r06_notes.md section 6; rounds 3 - 5 sent 8 KB0 + 1 pieces of 256 bytes here)
    constexpr int XPIECES = (DO + 1 + 7) / 8;
    constexpr int XLAND_BYTES = XPIECES * WV * 16;
    constexpr int WAVE_BYTES = LAND_BYTES + SPILL_BYTES + XLAND_BYTES;
    constexpr int LDS_TOTAL = WAVES * WAVE_BYTES + (INV_LDS ? OPS_BYTES : 0) + (TAIL_LDS ? 2 * TAILV * 4 : 0);
    static_assert(DO + 1 <= 32, "two k-blocks of inputs + the bias slot");
    static_assert(LDS_TOTAL >= WAVES * P * 4 && LDS_TOTAL <= 160 * 1024, "LDS budget; the fold rows alias the landing zones");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int wave = threadIdx.x / WV, lane = threadIdx.x % WV;
    const int lj = lane & 31, lh = lane >> 5;
    char* const land = smem + wave * WAVE_BYTES;
    char* const spill = land + LAND_BYTES;
    char* const xland = spill + SPILL_BYTES;
    char* const ops = smem + WAVES * WAVE_BYTES;                       // [N_OPS][3][64] x 16 B
    float* const tailv = reinterpret_cast<float*>(ops + (INV_LDS ? OPS_BYTES : 0));    // [2][TAILV]

    const int B = a.B;
    const int n_tiles = B / TS;
    const int wave_global = blockIdx.x * WAVES + wave;
    const int waves_total = gridDim.x * WAVES;

    // one tile ahead: the observation slots and the weight in registers, the cached activations by LDS-direct loads
    // (branch-free: a lane half beyond the inputs reads a clamped row and selects the constant)
    // The observations and the weight travel the same way as the activations, hidden from the compiler's wait-count
    // bookkeeping (a tracked load next to hidden ones would make every vmcnt(N) it computes wait for the younger hidden
    // loads too): lane L of piece p carries samples 4 (L & 7) .. + 3 of row 8 p + (L >> 3), so the piece lands row-major
    // [8 rows][32 samples] and take_x() reads x[d][sample] at (32 d + sample) floats, conflict-free.
    const unsigned xland_lds = __builtin_amdgcn_readfirstlane((unsigned)(size_t)(lptr_t)xland);
    auto fetch = [&](int tile, float (&)[KB0][8], float&) {
#pragma unroll
        for (int p = 0; p < XPIECES; ++p) {
            const int d = 8 * p + (lane >> 3);
            const float* g = (d < DO ? a.obs + (size_t)d * B : a.weight) + tile * TS + 4 * (lane & 7);
            asm volatile("s_mov_b32 m0, %1\n\tglobal_load_lds_dwordx4 %0, off" :: "v"(g), "s"(xland_lds + p * (WV * 16)) : "memory");
        }
    };
    auto take_x = [&](float (&xq)[KB0][8], float& wq) {
        const float* xl = reinterpret_cast<const float*>(xland) + lj;
#pragma unroll
        for (int kb = 0; kb < KB0; ++kb)
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int d = 16 * kb + 8 * lh + j;
                const float v = xl[32 * (d < DO ? d : DO)];
                xq[kb][j] = d < DO ? v : (d == DO ? 1.0f : 0.0f);
            }
        wq = xl[32 * DO];
    };
    // LDS byte address of this wavefront's landing zone (wave-uniform): M0 for rows 0..3, + 4096 for rows 4..7; the
    // instruction offset advances the global and the LDS address together (row q of a tile is 1 KB in both)
    const unsigned land_lds = __builtin_amdgcn_readfirstlane((unsigned)(size_t)(lptr_t)land);
    auto fetch_acts = [&](int tile) {
        const float* src = a.acts + ((size_t)tile * 8 * WV + lane) * 4;
        asm volatile("s_mov_b32 m0, %2\n\t"
                     "global_load_lds_dwordx4 %0, off\n\t"
                     "global_load_lds_dwordx4 %0, off offset:1024\n\t"
                     "global_load_lds_dwordx4 %0, off offset:2048\n\t"
                     "global_load_lds_dwordx4 %0, off offset:3072\n\t"
                     "s_mov_b32 m0, %3\n\t"
                     "global_load_lds_dwordx4 %1, off\n\t"
                     "global_load_lds_dwordx4 %1, off offset:1024\n\t"
                     "global_load_lds_dwordx4 %1, off offset:2048\n\t"
                     "global_load_lds_dwordx4 %1, off offset:3072"
                     :: "v"(src), "v"(src + 4 * WV * 4), "s"(land_lds), "s"(land_lds + 4096u) : "memory");
    };
    float xb[KB0][8], xb_next[KB0][8];
    float wgt = 0.0f, wgt_next = 0.0f;
    if (wave_global < n_tiles) {
        fetch(wave_global, xb_next, wgt_next);
        fetch_acts(wave_global);
    }
    asm volatile("" ::: "memory");   // (the first tile's inputs travel while the operands below are staged)

    const float* __restrict__ th = a.theta;
    const float* __restrict__ vc = a.vec;
    // ---- loop-invariant operands, split once per launch ------------------------------------------------------------------
    // operand block o: 0 .. KB0 - 1 = dW0^T (+ db0 in the bias slot), KB0 + kb = dW1^T, KB0 + 2 + kb = W1^T, KB0 + 4 + kb = W1
    auto make_op = [&](int o, Parts& out) {
        float t[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (o < KB0) {
                const int d = 16 * o + 8 * lh + j;           // A[i = lj][d] = dW0[d][i] (d < DO), db0[i] (d == DO)
                t[j] = d < DO ? vc[N::W0 + d * H + lj] : (d == DO ? vc[N::B0 + lj] : 0.0f);
            } else {
                const int q = o - KB0, kb = q & 1, u = frag_unit(8 * kb + j, lh);
                t[j] = q < 2 ? vc[N::W1 + u * H + lj]        // dW1^T: A[i][k] = dW1[k][i]
                     : q < 4 ? th[N::W1 + u * H + lj]        // W1^T
                             : th[N::W1 + lj * H + u];       // W1:    A[k][i] = W1[k][i]
            }
        }
        split8(t, out);
    };
    Parts R_ops[INV_LDS ? 1 : N_OPS];
    float R_db1[TAIL_LDS ? 1 : 16], R_W2[TAIL_LDS ? 1 : 16][DA], R_dW2[TAIL_LDS ? 1 : 16][DA];
    if constexpr (INV_LDS) {
        for (int o = wave; o < N_OPS; o += WAVES) {
            Parts t;
            make_op(o, t);
#pragma unroll
            for (int p = 0; p < 3; ++p) *reinterpret_cast<bf16x8*>(ops + ((o * 3 + p) * WV + lane) * 16) = t.p[p];
        }
    } else {
#pragma unroll
        for (int o = 0; o < N_OPS; ++o) make_op(o, R_ops[o]);
    }
    if constexpr (TAIL_LDS) {
        for (int e = threadIdx.x; e < 2 * 16; e += WAVES * WV) {
            const int hh = e / 16, r = e % 16, u = frag_unit(r, hh);
            float* tv = tailv + hh * TAILV;
#pragma unroll
            for (int k = 0; k < DA; ++k) {                 // [W2 column k | dW2 column k] rows of this half, then db1
                tv[k * 16 + r] = th[N::W2 + u * DA + k];
                tv[(DA + k) * 16 + r] = vc[N::W2 + u * DA + k];
            }
            tv[2 * DA * 16 + r] = vc[N::B1 + u];
        }
    } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int u = frag_unit(r, lh);
            R_db1[r] = vc[N::B1 + u];
#pragma unroll
            for (int k = 0; k < DA; ++k) { R_W2[r][k] = th[N::W2 + u * DA + k]; R_dW2[r][k] = vc[N::W2 + u * DA + k]; }
        }
    }
    if constexpr (TAIL_LDS) __syncthreads();
#if RL_ABL_OPS
    Parts abl_op;
    for (int p = 0; p < 3; ++p) abl_op.p[p] = *reinterpret_cast<const bf16x8*>(ops + (p * WV + lane) * 16);
#endif
    auto op = [&](int o) -> Parts {
#if RL_ABL_OPS
        if (o >= 0) { Parts t = abl_op; asm volatile("" : "+v"(t.p[0]), "+v"(t.p[1]), "+v"(t.p[2])); return t; }
#endif
        if constexpr (INV_LDS) {
            Parts t;
#pragma unroll
            for (int p = 0; p < 3; ++p) t.p[p] = *reinterpret_cast<const bf16x8*>(ops + ((o * 3 + p) * WV + lane) * 16);
            return t;
        } else {
            return R_ops[o];
        }
    };
    // acc += sum_kb op(base + kb) x Bk[kb] with the operand blocks read one AHEAD: `cur` holds block `base` (read by the
    // caller or by the previous chain), the block after the last one of this chain is `nxt_o` (< 0: none)
    auto chain_ahead = [&](int base, int nb, const Parts* Bk, f32x16 acc_, Parts& cur, int nxt_o) -> f32x16 {
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            if (kb < nb) {
                Parts nxtp = cur;
                const int o = kb + 1 < nb ? base + kb + 1 : nxt_o;
                if (o >= 0) nxtp = op(o);
                __builtin_amdgcn_sched_barrier(0);
                acc_ = mm6(cur, Bk[kb], acc_);
                cur = nxtp;
            }
        }
        return acc_;
    };
    // identity operands of the transpositions: B[k][n] = (k == n) in the k order of the fragment they meet
    bf16x8 Id[2], Idx[KB0];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        Id[0][j] = (__bf16)(frag_unit(j, lh) == lj ? 1.0f : 0.0f);
        Id[1][j] = (__bf16)(frag_unit(8 + j, lh) == lj ? 1.0f : 0.0f);
#pragma unroll
        for (int kb = 0; kb < KB0; ++kb) Idx[kb][j] = (__bf16)(16 * kb + 8 * lh + j == lj ? 1.0f : 0.0f);
    }
    float db2[DA], fk[DA], var_[DA];
    bool floored[DA];
#pragma unroll
    for (int k = 0; k < DA; ++k) {
        const float raw = th[N::LSTD + k];
        floored[k] = raw < a.log_min_std;
        const float ls = fmaxf(raw, a.log_min_std);
        var_[k] = __expf(2.0f * ls);
        fk[k] = 2.0f / (2.0f * var_[k] + 1e-8f);
        db2[k] = vc[N::B2 + k];
    }

    // ---- accumulators ---------------------------------------------------------------------------------------------
    f32x16 gW1, gW0;
    float gW2l[16][DA], gb1l[16], gb2[DA], wsum = 0.0f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        gW1[r] = 0.0f; gW0[r] = 0.0f; gb1l[r] = 0.0f;
#pragma unroll
        for (int k = 0; k < DA; ++k) gW2l[r][k] = 0.0f;
    }
#pragma unroll
    for (int k = 0; k < DA; ++k) gb2[k] = 0.0f;


    // every load the compiler knows of (parameters, tangent, the staging above) has landed before the loop is entered,
    // and it is told so with an instruction it models: otherwise the loop header inherits "loads may be pending" from
    // the preheader and a vmcnt(N) wait for a loop-invariant value survives inside the loop, where it would wait for
    // the hidden loads of the next tile
    __builtin_amdgcn_s_waitcnt(0x0F70);      // vmcnt(0), expcnt / lgkmcnt untouched
    for (int tile = wave_global; tile < n_tiles; tile += waves_total) {
        // ---- this tile's inputs; the next tile's start travelling ------------------------------------------------
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        f32x16 h0, h1;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const f32x4 v0 = *reinterpret_cast<const f32x4*>(land + (q * WV + lane) * 16);
            const f32x4 v1 = *reinterpret_cast<const f32x4*>(land + ((4 + q) * WV + lane) * 16);
#pragma unroll
            for (int e = 0; e < 4; ++e) { h0[4 * q + e] = v0[e]; h1[4 * q + e] = v1[e]; }
        }
        take_x(xb, wgt);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // the landing zone is in registers before it is refilled
        {   // the wavefront's last tile prefetches itself again (no branch in the loop body)
            const int nxt = tile + waves_total < n_tiles ? tile + waves_total : tile;
#if !RL_ABL_FETCH
            fetch(nxt, xb_next, wgt_next);
            fetch_acts(nxt);
#else
            (void)nxt;
#endif
        }
        // the output layer's rows of this lane half, read where they are used (two wavefronts per SIMD: from LDS)
        const float* tv = tailv + lh * TAILV;
        auto W2_ = [&](int r, int k) { if constexpr (TAIL_LDS) return tv[k * 16 + r]; else return R_W2[r][k]; };
        auto dW2_ = [&](int r, int k) { if constexpr (TAIL_LDS) return tv[(DA + k) * 16 + r]; else return R_dW2[r][k]; };
        auto db1_ = [&](int r) { if constexpr (TAIL_LDS) return tv[2 * DA * 16 + r]; else return R_db1[r]; };
        // keeps the LDS reads of a stage inside it (the compiler would otherwise start every loop-invariant read at the
        // top of the tile and hold 160 registers for them)
        auto stage = [&]() { if constexpr (TAIL_LDS) asm volatile("" ::: "memory"); };

        // ---- operands of this tile ---------------------------------------------------------------------------------------
        Parts opcur;
        if constexpr (INV_LDS) {              // the first operand block travels while the tile's inputs are split
            opcur = op(0);
            __builtin_amdgcn_sched_barrier(0);
        }
        Parts Xs[KB0], H0s[2];
#pragma unroll
        for (int kb = 0; kb < KB0; ++kb) split8(xb[kb], Xs[kb]);
        split_frag(h0, H0s);

        // ---- tangent forward: dmu = J v ---------------------------------------------------------------------------------
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
        if constexpr (INV_LDS) acc = chain_ahead(0, KB0, Xs, acc, opcur, KB0);    // dW0^T x + db0 (leaves block KB0 in opcur)
        else
#pragma unroll
        for (int kb = 0; kb < KB0; ++kb) acc = mm6(op(kb), Xs[kb], acc);          // dW0^T x + db0
        f32x16 dh0;
        times_dtanh(acc, h0, dh0);
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = db1_(r);
        if constexpr (INV_LDS) acc = chain_ahead(KB0, 2, H0s, acc, opcur, KB0 + 2);     // dW1^T h0 (leaves W1^T's first block)
        else
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) acc = mm6(op(KB0 + kb), H0s[kb], acc);       // dW1^T h0
        if constexpr (INV_LDS) {
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int p = 0; p < 3; ++p) *reinterpret_cast<bf16x8*>(spill + ((kb * 3 + p) * WV + lane) * 16) = H0s[kb].p[p];
        }
        stage();
        {
            Parts D0s[2];
            split_frag(dh0, D0s);
            if constexpr (INV_LDS) acc = chain_ahead(KB0 + 2, 2, D0s, acc, opcur, -1);  // W1^T dh0
            else
#pragma unroll
            for (int kb = 0; kb < 2; ++kb) acc = mm6(op(KB0 + 2 + kb), D0s[kb], acc);   // W1^T dh0
        }
        stage();
        const float c = wgt * a.inv_count;
        f32x16 dz1;
        float gmu[DA];
        f32x16 gz1;
        // the same sums with two fragment registers per instruction: the per-lane dot products of the output layer run
        // over register PAIRS (the two partial sums meet at the end), the outer-product and bias accumulators advance in pairs
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const f32x2 hh = pair_of(h1, j);
            const f32x2 d = __builtin_elementwise_fma(-hh, hh, f32x2{1.0f, 1.0f});
            set_pair(dz1, j, d);
            set_pair(acc, j, pair_of(acc, j) * d);                                // dh1
        }
        // rows r = 0 .. 15 of column k (which: 0 = W2, 1 = its tangent) of this lane half: four 16-byte reads (LDS) or moves
        auto rows_of = [&](int which, int k, f32x4 (&out_)[4]) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if constexpr (TAIL_LDS) out_[q] = *reinterpret_cast<const f32x4*>(tv + (which * DA + k) * 16 + 4 * q);
                else
#pragma unroll
                    for (int e = 0; e < 4; ++e) out_[q][e] = which ? R_dW2[4 * q + e][k] : R_W2[4 * q + e][k];
            }
        };
#pragma unroll
        for (int k = 0; k < DA; ++k) {
            f32x4 wq[4], dq[4];
            rows_of(0, k, wq);
            rows_of(1, k, dq);
            f32x2 pa[2], pb[2];
            pa[0] = pa[1] = pb[0] = pb[1] = f32x2{0.0f, 0.0f};
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int q = j >> 1, e = 2 * (j & 1);
                pa[j & 1] = __builtin_elementwise_fma(pair_of(h1, j), f32x2{dq[q][e], dq[q][e + 1]}, pa[j & 1]);
                pb[j & 1] = __builtin_elementwise_fma(pair_of(acc, j), f32x2{wq[q][e], wq[q][e + 1]}, pb[j & 1]);
            }
            const f32x2 pd = (pa[0] + pb[0]) + (pa[1] + pb[1]);
            const float dmu = db2[k] + half_sum_swap(pd[0] + pd[1]);
            gmu[k] = c * dmu * fk[k];
        }
        if (lh == 0) {
            wsum += c;
#pragma unroll
            for (int k = 0; k < DA; ++k) gb2[k] += gmu[k];
        }
        stage();
        // ---- back-propagation, sample-major ---------------------------------------------------------------------------------
        {
            f32x2 g[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) g[j] = f32x2{0.0f, 0.0f};
#pragma unroll
            for (int k = 0; k < DA; ++k) {
                f32x4 wq[4];
                rows_of(0, k, wq);
                const f32x2 gk = {gmu[k], gmu[k]};
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int q = j >> 1, e = 2 * (j & 1);
                    g[j] = __builtin_elementwise_fma(f32x2{wq[q][e], wq[q][e + 1]}, gk, g[j]);
                    const f32x2 w2 = __builtin_elementwise_fma(pair_of(h1, j), gk, f32x2{gW2l[2 * j][k], gW2l[2 * j + 1][k]});
                    gW2l[2 * j][k] = w2[0]; gW2l[2 * j + 1][k] = w2[1];
                }
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const f32x2 gz = g[j] * pair_of(dz1, j);
                set_pair(gz1, j, gz);
                const f32x2 b1n = f32x2{gb1l[2 * j], gb1l[2 * j + 1]} + gz;
                gb1l[2 * j] = b1n[0]; gb1l[2 * j + 1] = b1n[1];
            }
        }
        stage();
        if constexpr (INV_LDS) {
            opcur = op(KB0 + 4);
            __builtin_amdgcn_sched_barrier(0);
        }
        Parts G1s[2];
        split_frag(gz1, G1s);
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
        if constexpr (INV_LDS) acc = chain_ahead(KB0 + 4, 2, G1s, acc, opcur, -1);      // W1 gz1
        else
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) acc = mm6(op(KB0 + 4 + kb), G1s[kb], acc);       // W1 gz1
        stage();
        {
            if constexpr (INV_LDS) {
#pragma unroll
                for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                    for (int p = 0; p < 3; ++p) H0s[kb].p[p] = *reinterpret_cast<const bf16x8*>(spill + ((kb * 3 + p) * WV + lane) * 16);
            }
            Parts H0t[2], G1t[2];
            transpose_units(H0s, Id, H0t);                                        // h0 unit-major
            transpose_units(G1s, Id, G1t);
#pragma unroll
            for (int kb = 0; kb < 2; ++kb) gW1 = mm6(H0t[kb], G1t[kb], gW1);      // gW1 += h0^T gz1 (samples are K)
        }
        f32x16 gz0;
        times_dtanh(acc, h0, gz0);
        {
            Parts G0s[2], G0t[2], Xt[2];
            split_frag(gz0, G0s);
            transpose_units(G0s, Id, G0t);
            transpose_inputs<KB0>(Xs, Idx, Xt);
#pragma unroll
            for (int kb = 0; kb < 2; ++kb) gW0 = mm6(Xt[kb], G0t[kb], gW0);       // gW0 += x_ext^T gz0
        }
    }

    // the last tile's (redundant) prefetch is still travelling into this wavefront's landing zone, which the fold buffer
    // aliases: let it land first
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

    // ---- fold the wavefronts of this workgroup in a fixed order, write ONE partial row ----------------------------------
    // per-lane accumulators of the thin products: sum over the 32 samples of a lane half
    float b1s[16], w2s[16][DA];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        float v = gb1l[r];
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, WV);
        b1s[r] = v;
#pragma unroll
        for (int k = 0; k < DA; ++k) {
            float w = gW2l[r][k];
#pragma unroll
            for (int o = 16; o > 0; o >>= 1) w += __shfl_xor(w, o, WV);
            w2s[r][k] = w;
        }
    }
    float b2s[DA];
#pragma unroll
    for (int k = 0; k < DA; ++k) b2s[k] = wave_sum(gb2[k]);
    const float ws = wave_sum(wsum);
    __syncthreads();
    // every wavefront lays its contribution out as one row (each parameter has exactly one contributor per wavefront),
    // then the columns are summed in wavefront order -- the same sums as folding the wavefronts one after the other,
    // with two workgroup barriers instead of WAVES + 2
    float* const myrow = reinterpret_cast<float*>(smem) + wave * P;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int u = frag_unit(r, lh);
        myrow[N::W1 + u * H + lj] = gW1[r];                           // row = unit of h0, column = unit of gz1
        if (u < DO) myrow[N::W0 + u * H + lj] = gW0[r];               // row = input (or the bias slot)
        else if (u == DO) myrow[N::B0 + lj] = gW0[r];
    }
    if (lj == 0) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int u = frag_unit(r, lh);
            myrow[N::B1 + u] = b1s[r];
#pragma unroll
            for (int k = 0; k < DA; ++k) myrow[N::W2 + u * DA + k] = w2s[r][k];
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < DA; ++k) {
            myrow[N::B2 + k] = b2s[k];
            myrow[N::LSTD + k] = log_std_fisher(var_[k], floored[k]) * vc[N::LSTD + k] * ws;
        }
    }
    __syncthreads();
    fold_rows<WAVES, P>(smem, a.partial);
}

// =====================================================================================================================
// fvp_split64_kernel<DO, DA> -- the same product for two 64-unit tanh layers (BASELINE config C5's GaussianMLPPolicy(64, 64)),
// round 5.  policy_pass_kernel<Net<.., 64>, FVP> spends 17.8 k of its 41 k cycles per 32-sample tile in f32 matrix
// instructions that run at the vector rate; here every product is the six-term bf16 form of the kernel above (282 matrix
// instructions of 32 cycles per tile).  One wavefront per SIMD owns a tile (512 registers; the cooperative two-wavefront
// kernel of policy_csplit_kernels.hip pays seven workgroup barriers and an LDS hand-over per layer for the same tile and
// measured slower than the f32 kernel, profiles/r04_notes.md):
//   * fragments are arrays over the HT = 2 row tiles of a layer; a layer's B operand is 2 HT k-blocks of 16 units;
//   * all loop-invariant operands (28 blocks x 3 parts x 1 KB = 84 KB) live in LDS, read per use;
//   * the output layer's outer product gW2 += h1^T gmu does NOT accumulate per lane (32 units x DA values = 192 registers for
//     six actions): lane u (= unit u of the 64) walks the tile's 32 samples, reading h1[s][u] straight from the landing
//     zone of the cached fragments and the sample's cotangent gmu[s][.] from a 1 KB wave-private row buffer (broadcast
//     reads) -- DA accumulators per lane, no reduction over the lanes at the end;
//   * the next tile's fragments start travelling (LDS-direct loads) once that walk is done with the landing zone -- the
//     back-propagation, transpositions and outer products behind it cover the HBM round trip.
// Same inputs, same partial-row / float64 row reduction, a result that differs from the f32 kernel's by rounding only
// (tests/test_gpu_fvp_split.py, tests/test_gpu_update_parity.py run both).
template <int DO, int DA>
__global__ void __launch_bounds__(4 * WV, 1) fvp_split64_kernel(Args a) {
    constexpr int HT = 2, HH = 64;
    using N = Net<DO, DA, HH>;
    constexpr int P = N::P;
    constexpr int WAVES = 4;
    constexpr int KB0 = (DO + 1 + 15) / 16;        // k-blocks of the input layer (inputs + the bias slot)
    constexpr int KBH = 2 * HT;                    // k-blocks of a hidden layer's output (16 units each)
    constexpr int O_DW0 = 0, O_DW1 = O_DW0 + HT * KB0, O_W1T = O_DW1 + HT * KBH, O_W1 = O_W1T + HT * KBH,
                  N_OPS = O_W1 + HT * KBH;
    constexpr int OPS_BYTES = N_OPS * 3 * WV * 16;
    constexpr int TAILV = HT * 16 * DA * 2 + HT * 16;            // floats per lane half: W2 | dW2 | db1, [k][t][16 rows]
    constexpr int LAND64 = 2 * HH * TS * 4;                      // h0 | h1 fragments of one tile: 16 rows of 1 KB
    constexpr int GMU_BYTES = TS * 8 * 4;                        // [sample][8] cotangents on the mean (DA <= 8)
    constexpr int WAVE_BYTES = LAND64 + GMU_BYTES;
    constexpr int LDS_TOTAL = WAVES * WAVE_BYTES + OPS_BYTES + 2 * TAILV * 4;
    static_assert(DO + 1 <= 32 && DA <= 8, "two k-blocks of inputs + the bias slot; at most eight actions");
    static_assert(LDS_TOTAL >= WAVES * P * 4 && LDS_TOTAL <= 160 * 1024, "LDS budget; the fold rows alias everything");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int wave = threadIdx.x / WV, lane = threadIdx.x % WV;
    const int lj = lane & 31, lh = lane >> 5;
    char* const land = smem + wave * WAVE_BYTES;
    float* const gmub = reinterpret_cast<float*>(land + LAND64);
    char* const ops = smem + WAVES * WAVE_BYTES;
    float* const tailv = reinterpret_cast<float*>(ops + OPS_BYTES);

    const int B = a.B;
    const int n_tiles = B / TS;
    const int wave_global = blockIdx.x * WAVES + wave;
    const int waves_total = gridDim.x * WAVES;

    auto fetch = [&](int tile, float (&xq)[KB0][8], float& wq) {
        const int b = tile * TS + lj;
        wq = a.weight[b];
#pragma unroll
        for (int kb = 0; kb < KB0; ++kb)
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int d = 16 * kb + 8 * lh + j;
                const float v = a.obs[(size_t)(d < DO ? d : DO - 1) * B + b];
                xq[kb][j] = d < DO ? v : (d == DO ? 1.0f : 0.0f);
            }
    };
    auto fetch_acts = [&](int tile) {
        const float* src = a.acts + ((size_t)tile * (4 * 2 * HT) * WV + lane) * 4;
#pragma unroll
        for (int q = 0; q < 4 * 2 * HT; ++q)
            __builtin_amdgcn_global_load_lds((gptr_t)(src + q * WV * 4), (lptr_t)(land + q * WV * 16), 16, 0, 0);
    };
    float xb[KB0][8], xb_next[KB0][8];
    float wgt = 0.0f, wgt_next = 0.0f;
    if (wave_global < n_tiles) {
        fetch(wave_global, xb_next, wgt_next);
        fetch_acts(wave_global);
    }
    asm volatile("" ::: "memory");

    const float* __restrict__ th = a.theta;
    const float* __restrict__ vc = a.vec;
    // ---- loop-invariant operands, split once per launch, in LDS ------------------------------------------------------
    // block (row tile t, k-block): A[i = 32 t + lj][k-slot (lh, j)]
    for (int o = wave; o < N_OPS; o += WAVES) {
        float tv8[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (o < O_DW1) {                               // dW0^T (+ db0 in the bias slot): k = input 16 kb0 + 8 lh + j
                const int t = o / KB0, kb0 = o % KB0, i = 32 * t + lj, d = 16 * kb0 + 8 * lh + j;
                tv8[j] = d < DO ? vc[N::W0 + d * HH + i] : (d == DO ? vc[N::B0 + i] : 0.0f);
            } else {
                const int q = o - O_DW1, fam = q / (HT * KBH), r_ = q % (HT * KBH), t = r_ / KBH, kbg = r_ % KBH;
                const int i = 32 * t + lj, u = 32 * (kbg >> 1) + frag_unit(8 * (kbg & 1) + j, lh);
                tv8[j] = fam == 0 ? vc[N::W1 + u * HH + i]   // dW1^T: A[i][k] = dW1[k][i]
                       : fam == 1 ? th[N::W1 + u * HH + i]   // W1^T
                                  : th[N::W1 + i * HH + u];  // W1:    A[i][k] = W1[i][k]
            }
        }
        Parts tp;
        split8(tv8, tp);
#pragma unroll
        for (int p = 0; p < 3; ++p) *reinterpret_cast<bf16x8*>(ops + ((o * 3 + p) * WV + lane) * 16) = tp.p[p];
    }
    for (int e = threadIdx.x; e < 2 * HT * 16; e += WAVES * WV) {
        const int hh = e / (HT * 16), t = (e / 16) % HT, r = e % 16, u = 32 * t + frag_unit(r, hh);
        float* tv = tailv + hh * TAILV;
#pragma unroll
        for (int k = 0; k < DA; ++k) {
            tv[(k * HT + t) * 16 + r] = th[N::W2 + u * DA + k];
            tv[((DA + k) * HT + t) * 16 + r] = vc[N::W2 + u * DA + k];
        }
        tv[2 * DA * HT * 16 + t * 16 + r] = vc[N::B1 + u];
    }
    __syncthreads();
#if RL_ABL_OPS
    Parts abl_op64;
    for (int p = 0; p < 3; ++p) abl_op64.p[p] = *reinterpret_cast<const bf16x8*>(ops + (p * WV + lane) * 16);
#endif
    auto op = [&](int o) -> Parts {
#if RL_ABL_OPS
        if (o >= 0) { Parts t = abl_op64; asm volatile("" : "+v"(t.p[0]), "+v"(t.p[1]), "+v"(t.p[2])); return t; }
#endif
        Parts t;
#pragma unroll
        for (int p = 0; p < 3; ++p) t.p[p] = *reinterpret_cast<const bf16x8*>(ops + ((o * 3 + p) * WV + lane) * 16);
        return t;
    };
    // acc[t] += (operand blocks base + t * NKB + kb) x Bk[kb] for both row tiles: ONE stream of 2 NKB block products that
    // alternates the row tiles (two independent accumulator chains on the matrix pipe) with the NEXT block's three parts
    // read from LDS before the current block's six products are issued -- a lone wavefront has nobody to hide an LDS round
    // trip behind (first build: 28 exposed round trips per tile here)
    auto chains = [&](int base, const auto& Bk, f32x16 (&acc_)[HT]) {
        constexpr int NKB = sizeof(Bk) / sizeof(Parts);
        Parts cur = op(base);
#pragma unroll
        for (int i = 0; i < NKB * HT; ++i) {
            const int kb = i / HT, t = i % HT;
            Parts nxtp = cur;
            if (i + 1 < NKB * HT) nxtp = op(base + ((i + 1) % HT) * NKB + (i + 1) / HT);
            __builtin_amdgcn_sched_barrier(0);
            acc_[t] = mm6(cur, Bk[kb], acc_[t]);
            cur = nxtp;
        }
    };
    bf16x8 Id[2], Idx[KB0];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        Id[0][j] = (__bf16)(frag_unit(j, lh) == lj ? 1.0f : 0.0f);
        Id[1][j] = (__bf16)(frag_unit(8 + j, lh) == lj ? 1.0f : 0.0f);
#pragma unroll
        for (int kb = 0; kb < KB0; ++kb) Idx[kb][j] = (__bf16)(16 * kb + 8 * lh + j == lj ? 1.0f : 0.0f);
    }
    float db2[DA], fk[DA], var_[DA];
    bool floored[DA];
#pragma unroll
    for (int k = 0; k < DA; ++k) {
        const float raw = th[N::LSTD + k];
        floored[k] = raw < a.log_min_std;
        const float ls = fmaxf(raw, a.log_min_std);
        var_[k] = __expf(2.0f * ls);
        fk[k] = 2.0f / (2.0f * var_[k] + 1e-8f);
        db2[k] = vc[N::B2 + k];
    }
    // where lane u = lane finds h1[s][u] in the landing zone: row (HT + t) * 4 + (r >> 2) of 1 KB, lane slot s + 32 half,
    // element r & 3, with u = 32 t + frag_unit(r, half)
    const int h1_off = (((HT + (lane >> 5)) * 4 + ((lane & 31) >> 3)) * WV + 32 * ((lane & 7) >> 2)) * 16 + (lane & 3) * 4;

    // ---- accumulators ---------------------------------------------------------------------------------------------
    f32x16 gW1[HT][HT], gW0[HT];
    float gb1l[HT][16], gW2u[DA], gb2[DA], wsum = 0.0f;
#pragma unroll
    for (int t = 0; t < HT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            gW0[t][r] = 0.0f; gb1l[t][r] = 0.0f;
#pragma unroll
            for (int t2 = 0; t2 < HT; ++t2) gW1[t][t2][r] = 0.0f;
        }
#pragma unroll
    for (int k = 0; k < DA; ++k) { gb2[k] = 0.0f; gW2u[k] = 0.0f; }

    for (int tile = wave_global; tile < n_tiles; tile += waves_total) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        f32x16 h0[HT], h1[HT];
#pragma unroll
        for (int t = 0; t < HT; ++t)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const f32x4 v0 = *reinterpret_cast<const f32x4*>(land + ((t * 4 + q) * WV + lane) * 16);
                const f32x4 v1 = *reinterpret_cast<const f32x4*>(land + (((HT + t) * 4 + q) * WV + lane) * 16);
#pragma unroll
                for (int e = 0; e < 4; ++e) { h0[t][4 * q + e] = v0[e]; h1[t][4 * q + e] = v1[e]; }
            }
#pragma unroll
        for (int kb = 0; kb < KB0; ++kb)
#pragma unroll
            for (int j = 0; j < 8; ++j) xb[kb][j] = xb_next[kb][j];
        wgt = wgt_next;
        const int nxt = tile + waves_total < n_tiles ? tile + waves_total : tile;
        fetch(nxt, xb_next, wgt_next);
        const float* tv = tailv + lh * TAILV;
        auto stage = [&]() { asm volatile("" ::: "memory"); };

        // ---- operands of this tile ---------------------------------------------------------------------------------------
        Parts Xs[KB0], H0s[KBH];
#pragma unroll
        for (int kb = 0; kb < KB0; ++kb) split8(xb[kb], Xs[kb]);
#pragma unroll
        for (int t = 0; t < HT; ++t) {
            Parts tmp[2];
            split_frag(h0[t], tmp);
            H0s[2 * t] = tmp[0]; H0s[2 * t + 1] = tmp[1];
        }

        // ---- tangent forward -----------------------------------------------------------------------------------------------
        f32x16 acc[HT], dh0[HT];
#pragma unroll
        for (int t = 0; t < HT; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;
        chains(O_DW0, Xs, acc);                                                            // dW0^T x + db0
#pragma unroll
        for (int t = 0; t < HT; ++t) times_dtanh(acc[t], h0[t], dh0[t]);
        stage();
        {
            // b1's tangent initialises the accumulators: the rows of this lane half in two bulk reads per row tile
            f32x4 bq[HT][4];
#pragma unroll
            for (int t = 0; t < HT; ++t)
#pragma unroll
                for (int q = 0; q < 4; ++q) bq[t][q] = *reinterpret_cast<const f32x4*>(tv + 2 * DA * HT * 16 + t * 16 + 4 * q);
#pragma unroll
            for (int t = 0; t < HT; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[t][r] = bq[t][r >> 2][r & 3];
        }
        chains(O_DW1, H0s, acc);                                                           // dW1^T h0
        stage();
        {
            Parts D0s[KBH];
#pragma unroll
            for (int t = 0; t < HT; ++t) {
                Parts tmp[2];
                split_frag(dh0[t], tmp);
                D0s[2 * t] = tmp[0]; D0s[2 * t + 1] = tmp[1];
            }
            chains(O_W1T, D0s, acc);                                                       // W1^T dh0
        }
        stage();
        const float c = wgt * a.inv_count;
        f32x16 dz1[HT], gz1[HT];
        float gmu[DA];
#pragma unroll
        for (int t = 0; t < HT; ++t)
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const f32x2 hh = pair_of(h1[t], j);
                const f32x2 d = __builtin_elementwise_fma(-hh, hh, f32x2{1.0f, 1.0f});
                set_pair(dz1[t], j, d);
                set_pair(acc[t], j, pair_of(acc[t], j) * d);                          // dh1
            }
#ifndef RL_ABL_THIN
#define RL_ABL_THIN 0          // timing ablation: the output layer's thin products and the gW2 walk left out (wrong results)
#endif
#if RL_ABL_THIN
#pragma unroll
        for (int k = 0; k < DA; ++k) gmu[k] = c * db2[k];
#pragma unroll
        for (int t = 0; t < HT; ++t) gz1[t] = acc[t];
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        fetch_acts(nxt);
#else
        // the output layer's rows of this lane half come in bulk: per action the 2 x 16 rows of W2 and of its tangent are
        // sixteen 16-byte reads issued together, waited for once (a scalar read per use exposed ~190 LDS round trips per tile)
        auto rows_of = [&](int which, int k, f32x4 (&out_)[HT][4]) {       // which: 0 = W2, 1 = dW2
#pragma unroll
            for (int t = 0; t < HT; ++t)
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    out_[t][q] = *reinterpret_cast<const f32x4*>(tv + ((which * DA + k) * HT + t) * 16 + 4 * q);
        };
#pragma unroll
        for (int k = 0; k < DA; ++k) {
            f32x4 wq[HT][4], dq[HT][4];
            rows_of(0, k, wq);
            rows_of(1, k, dq);
            // four independent partial sums (a dependent packed multiply-add costs a lone wavefront a wait state)
            f32x2 pa[HT], pb[HT];
#pragma unroll
            for (int t = 0; t < HT; ++t) pa[t] = pb[t] = f32x2{0.0f, 0.0f};
#pragma unroll
            for (int j = 0; j < 8; ++j)
#pragma unroll
                for (int t = 0; t < HT; ++t) {
                    const int q = j >> 1, e = 2 * (j & 1);
                    pa[t] = __builtin_elementwise_fma(pair_of(h1[t], j), f32x2{dq[t][q][e], dq[t][q][e + 1]}, pa[t]);
                    pb[t] = __builtin_elementwise_fma(pair_of(acc[t], j), f32x2{wq[t][q][e], wq[t][q][e + 1]}, pb[t]);
                }
            const f32x2 pd = (pa[0] + pb[0]) + (pa[1] + pb[1]);
            const float dmu = db2[k] + half_sum_swap(pd[0] + pd[1]);
            gmu[k] = c * dmu * fk[k];
        }
        if (lh == 0) {
            wsum += c;
#pragma unroll
            for (int k = 0; k < DA; ++k) { gb2[k] += gmu[k]; gmub[lj * 8 + k] = gmu[k]; }
        }
        // ---- back-propagation through the output layer, sample-major --------------------------------------------------
        {
            f32x2 g[HT][8];
#pragma unroll
            for (int t = 0; t < HT; ++t)
#pragma unroll
                for (int j = 0; j < 8; ++j) g[t][j] = f32x2{0.0f, 0.0f};
#pragma unroll
            for (int k = 0; k < DA; ++k) {
                f32x4 wq[HT][4];
                rows_of(0, k, wq);
                const f32x2 gk = {gmu[k], gmu[k]};
#pragma unroll
                for (int t = 0; t < HT; ++t)
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const int q = j >> 1, e = 2 * (j & 1);
                        g[t][j] = __builtin_elementwise_fma(f32x2{wq[t][q][e], wq[t][q][e + 1]}, gk, g[t][j]);
                    }
            }
#pragma unroll
            for (int t = 0; t < HT; ++t)
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const f32x2 gz = g[t][j] * pair_of(dz1[t], j);
                    set_pair(gz1[t], j, gz);
                    const f32x2 b1n = f32x2{gb1l[t][2 * j], gb1l[t][2 * j + 1]} + gz;
                    gb1l[t][2 * j] = b1n[0]; gb1l[t][2 * j + 1] = b1n[1];
                }
        }
        // ---- gW2 += h1^T gmu with the UNITS on the lanes: lane u walks the tile's samples ---------------------------------
        wave_sync();                                                   // the cotangent rows are in the buffer
        {
            const char* hp = land + h1_off;
#pragma unroll 8
            for (int s_ = 0; s_ < TS; ++s_) {
                const float hv = *reinterpret_cast<const float*>(hp + s_ * 16);
                const f32x4 g0 = *reinterpret_cast<const f32x4*>(gmub + s_ * 8);
                const f32x4 g1 = *reinterpret_cast<const f32x4*>(gmub + s_ * 8 + 4);
#pragma unroll
                for (int k = 0; k < DA; ++k) gW2u[k] = __builtin_fmaf(hv, k < 4 ? g0[k] : g1[k - 4], gW2u[k]);
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");       // the landing zone has been read: refill it
        fetch_acts(nxt);
#endif
        stage();
        Parts G1s[KBH];
#pragma unroll
        for (int t = 0; t < HT; ++t) {
            Parts tmp[2];
            split_frag(gz1[t], tmp);
            G1s[2 * t] = tmp[0]; G1s[2 * t + 1] = tmp[1];
        }
#pragma unroll
        for (int t = 0; t < HT; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;
        chains(O_W1, G1s, acc);                                                            // W1 gz1
        stage();
        {
            Parts H0t[HT][2], G1t[HT][2];
#pragma unroll
            for (int t = 0; t < HT; ++t) {
                const Parts hs[2] = {H0s[2 * t], H0s[2 * t + 1]}, gs[2] = {G1s[2 * t], G1s[2 * t + 1]};
                transpose_units(hs, Id, H0t[t]);
                transpose_units(gs, Id, G1t[t]);
            }
#pragma unroll
            for (int ti = 0; ti < HT; ++ti)
#pragma unroll
                for (int tj2 = 0; tj2 < HT; ++tj2)
#pragma unroll
                    for (int kb = 0; kb < 2; ++kb) gW1[ti][tj2] = mm6(H0t[ti][kb], G1t[tj2][kb], gW1[ti][tj2]);   // gW1 += h0^T gz1
        }
        stage();
        {
            Parts G0t[HT][2], Xt[2];
#pragma unroll
            for (int t = 0; t < HT; ++t) {
                f32x16 gz0;
                times_dtanh(acc[t], h0[t], gz0);
                Parts gs[2];
                split_frag(gz0, gs);
                transpose_units(gs, Id, G0t[t]);
            }
            transpose_inputs<KB0>(Xs, Idx, Xt);
#pragma unroll
            for (int t = 0; t < HT; ++t)
#pragma unroll
                for (int kb = 0; kb < 2; ++kb) gW0[t] = mm6(Xt[kb], G0t[t][kb], gW0[t]);                     // gW0 += x_ext^T gz0
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

    // ---- fold the wavefronts of this workgroup in a fixed order, write ONE partial row ----------------------------------
    float b1s[HT][16];
#pragma unroll
    for (int t = 0; t < HT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            float v = gb1l[t][r];
#pragma unroll
            for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, WV);
            b1s[t][r] = v;
        }
    float b2s[DA];
#pragma unroll
    for (int k = 0; k < DA; ++k) b2s[k] = wave_sum(gb2[k]);
    const float ws = wave_sum(wsum);
    __syncthreads();
    float* const myrow = reinterpret_cast<float*>(smem) + wave * P;
#pragma unroll
    for (int ti = 0; ti < HT; ++ti)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int u = 32 * ti + frag_unit(r, lh);
#pragma unroll
            for (int tj2 = 0; tj2 < HT; ++tj2) myrow[N::W1 + u * HH + 32 * tj2 + lj] = gW1[ti][tj2][r];
        }
#pragma unroll
    for (int t = 0; t < HT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int d = frag_unit(r, lh);
            if (d < DO) myrow[N::W0 + d * HH + 32 * t + lj] = gW0[t][r];
            else if (d == DO) myrow[N::B0 + 32 * t + lj] = gW0[t][r];
        }
    if (lj == 0) {
#pragma unroll
        for (int t = 0; t < HT; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) myrow[N::B1 + 32 * t + frag_unit(r, lh)] = b1s[t][r];
    }
#pragma unroll
    for (int k = 0; k < DA; ++k) myrow[N::W2 + lane * DA + k] = gW2u[k];               // lane = unit
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < DA; ++k) {
            myrow[N::B2 + k] = b2s[k];
            myrow[N::LSTD + k] = log_std_fisher(var_[k], floored[k]) * vc[N::LSTD + k] * ws;
        }
    }
    __syncthreads();
    fold_rows<WAVES, P>(smem, a.partial);
}

template <int DO, int DA>
static int launch64(const rl_policy_batch* g, const float* vec, void* ws, size_t ws_bytes, double* out, hipStream_t st) {
    constexpr int HT = 2, WAVES = 4;               // one wavefront per SIMD
    constexpr int KB0 = (DO + 1 + 15) / 16;
    constexpr int N_OPS = HT * KB0 + 3 * HT * 2 * HT;
    constexpr int LDS_BYTES = WAVES * (2 * 64 * TS * 4 + TS * 8 * 4) + N_OPS * 3 * WV * 16 + 2 * (HT * 16 * DA * 2 + HT * 16) * 4;
    return launch_tiles<fvp_split64_kernel<DO, DA>, WAVES, TS, LDS_BYTES, Net<DO, DA, 64>::P>("fvp_split64_kernel", make_args<Args>(g, vec),
                                                                                            ws, ws_bytes, out, st);
}

template <int DO, int DA, int WPS>
static int launch(const rl_policy_batch* g, const float* vec, void* ws, size_t ws_bytes, double* out, hipStream_t st) {
    constexpr int WAVES = 4 * WPS;
    constexpr int KB0 = (DO + 1 + 15) / 16;
    constexpr int LDS_BYTES = WAVES * (LAND_BYTES + (WPS == 2 ? 2 * 3 * WV * 16 : 0) + ((DO + 1 + 7) / 8) * WV * 16) +
                              (WPS == 2 ? ops_bytes(KB0) : 0) +
                              ((WPS == 2 || DA > 2) ? 2 * (16 * DA * 2 + 16) * 4 : 0);
    return launch_tiles<fvp_split_kernel<DO, DA, WPS>, WAVES, TS, LDS_BYTES, Net<DO, DA, H>::P>("fvp_split_kernel", make_args<Args>(g, vec),
                                                                                              ws, ws_bytes, out, st);
}

}  // namespace split

// The split product takes a cached Fisher-vector product of a two-layer 32-unit tanh net whose batch is a whole number
// of tiles; everything else stays on policy_pass_kernel.  rl_launch_opts.fvp_split = 1 switches it off (A/B runs, tests of
// the bit-identical cached / recomputed pair).  Returns RL_SPLIT_NOT_TAKEN when the launch is not its to make.
bool split_fvp_takes(const rl_policy_batch* g) {
    if (!g->activations || g->hidden2 != 0 || g->hidden0 != g->hidden1 || (g->hidden0 != 32 && g->hidden0 != 64) ||
        g->activation != RL_ACT_TANH || g->layer_activations != 0 || g->n_samples <= 0 || g->n_samples % TS != 0)
        return false;
    const int req = g->opts ? g->opts->fvp_split : 0;          // 0: the library's choice, 1: f32 matrix instructions, 2: cooperative
    if (req == 1) return false;
    if (g->hidden0 == 64) {
        if (req == 2) return false;                // (the tests of the cooperative class run every shape on THAT kernel)
#define SPLITCASE(DO, DA) if (g->obs_dim == DO && g->act_dim == DA) return true;
        SPLIT64_SHAPES(SPLITCASE)
#undef SPLITCASE
        return false;
    }
#define SPLITCASE(DO, DA) if (g->obs_dim == DO && g->act_dim == DA) return true;
    SPLIT_SHAPES(SPLITCASE)
#undef SPLITCASE
    return false;
}
int split_fvp_dispatch(const rl_policy_batch* g, const float* vec, void* ws, size_t ws_bytes, double* out, hipStream_t st) {
    if (!split_fvp_takes(g)) return RL_SPLIT_NOT_TAKEN;
    // two wavefronts per SIMD (operands in LDS) unless rl_launch_opts.fvp_split_wps = 1 asks for the one-wavefront, register-resident form
    if (g->hidden0 == 64) {
#define SPLITCASE(DO, DA) if (g->obs_dim == DO && g->act_dim == DA) return split::launch64<DO, DA>(g, vec, ws, ws_bytes, out, st);
        SPLIT64_SHAPES(SPLITCASE)
#undef SPLITCASE
        return RL_SPLIT_NOT_TAKEN;
    }
    const bool one = g->opts && g->opts->fvp_split_wps == 1;
#define SPLITCASE(DO, DA) if (g->obs_dim == DO && g->act_dim == DA) { \
        if constexpr (DA > 2) return split::launch<DO, DA, 1>(g, vec, ws, ws_bytes, out, st); \
        else return one ? split::launch<DO, DA, 1>(g, vec, ws, ws_bytes, out, st) : split::launch<DO, DA, 2>(g, vec, ws, ws_bytes, out, st); }
    SPLIT_SHAPES(SPLITCASE)
#undef SPLITCASE
    return RL_SPLIT_NOT_TAKEN;
}

}  // namespace rl
