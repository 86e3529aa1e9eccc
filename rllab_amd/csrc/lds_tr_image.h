// lds_tr_image.h -- address maps of the LDS image through which a wavefront turns a sample-major f16 fragment part into
// a unit-major one with ds_read_b64_tr_b16 (gfx950) instead of a product with an identity on the matrix pipe
// (policy_splith_kernels.hip).  Plain constexpr integer functions, no HIP types: tests/test_lds_tr_image_host.py includes
// this file in a host program that emulates a wavefront's stores and transposed reads on them.
//
// One part (hi or lo') of a 32-sample x 32-unit fragment is 2 KB: 256 chunks of 8 bytes, chunk (s, c) = the values of
// sample s at units 4c .. 4c + 3.  The instruction asks only that a lane's address be 8-byte aligned and point at four
// consecutive units of one sample, so where a chunk lies is free.  It lies at 8 x slot, the bits of slot being, low to high,
//     c1 | s0 | s1 | s2 ^ c0 | s3 | c2 | s4 | c0                      (s = s4..s0 the sample, c = c2 c1 c0 the unit quad)
// chosen so that BOTH sides address it as  (one register of the lane) + (a constant of the instruction):
//   the writer, lane (sample lj, half lh), holds for k-block kb the units frag_unit(8 kb + j, lh), j = 0..7 -- the quads
//     c = 4 kb + lh and c + 2.  They differ in c1, the lowest bit: ONE 16-byte store of the lane's eight f16 as they
//     stand, at tr_store_lane(lane) + TR_KB_STORE * kb  (c2 = kb has a bit of its own);
//   the reader, lane (unit lj, half lh), must receive for k-block kb in element j the value of sample
//     frag_unit(8 kb + j, lh) -- what a product with the identity + a repacking hands it: two transposed reads t = 0, 1 of
//     samples 16 kb + 8 t + 4 lh + q, q = 0..3, at tr_read_lane(lane) + TR_KB_READ * kb + TR_T_READ * t  (s4 = kb, s3 = t).
//     Within a 16-lane group, lane 4q + p supplies the address of row (sample) q, columns (units) 4p .. 4p + 3 of the
//     group's 16 units, and lane i receives column i with row q in element q.
// Banks: a 32-lane half of the transposed read (bank (addr / 4) % 64) varies s0 s1 c0 c1 c2 and finds four of them in the
// low five slot bits: 2-way.  The 16-byte store is served in groups of eight consecutive lanes (bank (addr / 4) % 32):
// s0 s1 s2 vary, slot bits 1..3 -- no conflict; over a 32-lane half with 64 banks it is the 2-way that 512 bytes must be.
// With plain 64-byte rows the reads are free of conflicts and the stores 8-way; no assignment of bits is free of
// conflicts on both sides unless the instruction's constant is XORed into the address, which costs a register or a
// vector instruction per access.
//
// The observation operand ([sample][input], rows of 32 inputs of which 16 KB0 are real; not used by the kernels at
// present, see profiles/fvp_lds_transpose_notes.md) takes the same image: a lane holds for k-block kb the inputs
// 16 kb + 8 lh + j -- the quads c = 4 kb + 2 lh and c + 1, two 8-byte stores at tr_chunk_offset(lj, c); quads from 4 KB0
// up are stored as zeros, so that the rows beyond the real inputs read as zeros from the image, not from masked lanes.
#pragma once

namespace rl {
namespace lds_tr {

constexpr int TR_PART_BYTES = 2048;      // one part of a 32 x 32 fragment
constexpr int TR_KB_STORE = 256;         // writer: k-block kb -> c2
constexpr int TR_KB_READ = 512;          // reader: k-block kb -> s4
constexpr int TR_T_READ = 128;           // reader: second run of four samples -> s3

// byte offset of chunk (sample s, unit quad c) in a part
constexpr int tr_chunk_offset(int s, int c) {
    return 8 * (((c >> 1) & 1) | ((s & 3) << 1) | ((((s >> 2) ^ c) & 1) << 3) | (((s >> 3) & 1) << 4) | (((c >> 2) & 1) << 5) |
                (((s >> 4) & 1) << 6) | ((c & 1) << 7));
}
// writer, lane = sample + 32 half: the 16-byte store of k-block 0 (quads `half` and `half + 2`)
constexpr int tr_store_lane(int lane) { return tr_chunk_offset(lane & 31, lane >> 5); }
// reader, lane = unit + 32 half: the transposed read (k-block 0, t = 0): row q = (lane & 15) >> 2 of the block, quad p = lane & 3
// of the 16-lane group's units
constexpr int tr_read_lane(int lane) { return tr_chunk_offset(4 * (lane >> 5) + ((lane & 15) >> 2), 4 * ((lane >> 4) & 1) + (lane & 3)); }

}  // namespace lds_tr
}  // namespace rl
