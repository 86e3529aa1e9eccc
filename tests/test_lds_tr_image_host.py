"""csrc/lds_tr_image.h, the address maps behind the transposed LDS reads of csrc/policy_splith_kernels.hip, on the host: a
stand-alone C++ program (g++, as tests/test_capi_symbols.py builds its C one) includes the header and policy_mfma.h's own
frag_unit, and emulates ONE wavefront on a 4 KB byte array in which every one of the 2 x 32 x 32 part values is distinct:

  * the stores of all 64 lanes (one 16-byte store per part and k-block for a 32-unit fragment; two 8-byte stores for the
    observation operand, the quads beyond its 16 KB0 real inputs stored as zeros);
  * ds_read_b64_tr_b16 as the ISA states it: per group of 16 consecutive lanes, lane 4q + p supplies the address of row q,
    columns 4p .. 4p + 3, and lane i receives column i with row q in element q.

It asserts that lane (unit lj, half lh) receives, for both k-blocks and both parts, in element j the value of sample
frag_unit(8 kb + j, lh) at unit lj -- what a product with an identity on the matrix pipe followed by pack_exact hands the
sample-contracted products; the same for the observation operand at KB0 = 1 and 2, with zeros beyond the real rows; that
every store is naturally aligned, every read address 8-byte aligned, all inside the wave's 4 KB, every byte written exactly
once; and, by the bank rule (bank = (addr / 4) % 64 over a 32-lane half; for the stores also over the lane groups and the
32 banks that serve them), that neither the stores nor the reads are worse than 2-way.  The program stands alone (its own
main, the image an array of exactly 4 KB), so the same source can be built with -fsanitize=address,undefined and run by hand."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rllab_amd", "csrc")

PROGRAM = r'''
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <map>
#include <set>
#include <vector>
#include "lds_tr_image.h"
@FRAG_UNIT@
using namespace rl::lds_tr;

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { if (fails++ < 20) { std::printf("FAIL %s:%d: ", #c, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

constexpr int IMG = 2 * TR_PART_BYTES, WV = 64;
struct Access { int lane, addr, bytes; };

struct Wave {
    std::vector<uint8_t> mem = std::vector<uint8_t>(IMG, 0xEE);     // exactly the wave's region: the sanitizer sees one byte past it
    std::vector<int> written = std::vector<int>(IMG, 0);
    void store(const Access& a, const uint16_t* v) {
        CHECK(a.addr >= 0 && a.addr + a.bytes <= IMG, "store of lane %d at %d", a.lane, a.addr);
        CHECK(a.addr % a.bytes == 0, "store of lane %d at %d not %d-byte aligned", a.lane, a.addr, a.bytes);
        if (a.addr < 0 || a.addr + a.bytes > IMG) return;
        std::memcpy(&mem[a.addr], v, a.bytes);
        for (int b = 0; b < a.bytes; ++b) ++written[a.addr + b];
    }
    // ds_read_b64_tr_b16: addr[64] in, out[64][4]
    void read_tr(const int* addr, uint16_t (*out)[4]) {
        for (int l = 0; l < WV; ++l) {
            CHECK(addr[l] >= 0 && addr[l] + 8 <= IMG, "read of lane %d at %d", l, addr[l]);
            CHECK(addr[l] % 8 == 0, "read of lane %d at %d not 8-byte aligned", l, addr[l]);
        }
        for (int g = 0; g < 4; ++g)
            for (int i = 0; i < 16; ++i)
                for (int q = 0; q < 4; ++q) {
                    const int a = addr[16 * g + 4 * q + (i >> 2)] + 2 * (i & 3);     // row q, column i of the group's block
                    uint16_t v = 0xDEAD;
                    if (a >= 0 && a + 2 <= IMG) std::memcpy(&v, &mem[a], 2);
                    out[16 * g + i][q] = v;
                }
    }
    void every_byte_once() {
        for (int b = 0; b < IMG; ++b) CHECK(written[b] == 1, "byte %d written %d times", b, written[b]);
    }
};

// the worst number of distinct dwords on one bank among the lanes of a group (groups of `group` consecutive lanes)
static int ways(const std::vector<Access>& acc, int group, int banks) {
    int worst = 0;
    for (int g0 = 0; g0 < WV; g0 += group) {
        std::map<int, std::set<int>> on;
        for (const Access& a : acc)
            if (a.lane >= g0 && a.lane < g0 + group)
                for (int d = a.addr / 4; d < (a.addr + a.bytes) / 4; ++d) on[d % banks].insert(d);
        for (auto& kv : on) worst = (int)kv.second.size() > worst ? (int)kv.second.size() : worst;
    }
    return worst;
}

static uint16_t value(int part, int s, int u) { return (uint16_t)(1 + 1024 * part + 32 * s + u); }    // 2048 distinct, none zero

// reads of one operand: every lane's elements against want(part, sample, column)
template <class F>
static void check_reads(Wave& w, F want, const char* what) {
    for (int part = 0; part < 2; ++part)
        for (int kb = 0; kb < 2; ++kb)
            for (int t = 0; t < 2; ++t) {
                int addr[WV];
                std::vector<Access> acc;
                for (int l = 0; l < WV; ++l) {
                    addr[l] = TR_PART_BYTES * part + tr_read_lane(l) + TR_KB_READ * kb + TR_T_READ * t;
                    acc.push_back({l, addr[l], 8});
                    const int lh = l >> 5, g2 = (l >> 4) & 1, q = (l & 15) >> 2, p = l & 3;
                    CHECK(addr[l] == TR_PART_BYTES * part + tr_chunk_offset(16 * kb + 8 * t + 4 * lh + q, 4 * g2 + p),
                          "%s: read address of lane %d is not its chunk's", what, l);
                }
                uint16_t out[WV][4];
                w.read_tr(addr, out);
                for (int l = 0; l < WV; ++l)
                    for (int q = 0; q < 4; ++q) {
                        const int lj = l & 31, lh = l >> 5, j = 4 * t + q, s = frag_unit(8 * kb + j, lh);
                        CHECK(out[l][q] == want(part, s, lj), "%s: part %d k-block %d lane %d element %d: got %d, want sample %d column %d = %d",
                              what, part, kb, l, j, out[l][q], s, lj, want(part, s, lj));
                    }
                CHECK(ways(acc, 32, 64) <= 2, "%s: transposed read %d-way", what, ways(acc, 32, 64));
            }
}

int main() {
    {   // a 32-sample x 32-unit fragment: lane (sample lj, half lh) holds units frag_unit(8 kb + j, lh)
        Wave w;
        for (int part = 0; part < 2; ++part)
            for (int kb = 0; kb < 2; ++kb) {
                std::vector<Access> acc;
                for (int l = 0; l < WV; ++l) {
                    const int lj = l & 31, lh = l >> 5;
                    uint16_t v[8];
                    for (int j = 0; j < 8; ++j) v[j] = value(part, lj, frag_unit(8 * kb + j, lh));
                    const Access a = {l, TR_PART_BYTES * part + tr_store_lane(l) + TR_KB_STORE * kb, 16};
                    CHECK(tr_store_lane(l) + TR_KB_STORE * kb == tr_chunk_offset(lj, 4 * kb + lh) &&
                          tr_store_lane(l) + TR_KB_STORE * kb + 8 == tr_chunk_offset(lj, 4 * kb + lh + 2), "store of lane %d is not its two chunks", l);
                    w.store(a, v);
                    acc.push_back(a);
                }
                CHECK(ways(acc, 8, 32) <= 2, "16-byte store %d-way over its groups of eight lanes", ways(acc, 8, 32));
                CHECK(ways(acc, 32, 64) <= 2, "16-byte store %d-way over a 32-lane half", ways(acc, 32, 64));
            }
        w.every_byte_once();
        check_reads(w, [](int part, int s, int u) { return value(part, s, u); }, "units");
    }
    for (int KB0 = 1; KB0 <= 2; ++KB0) {   // observations: lane (sample lj, half lh) holds inputs 16 kb + 8 lh + j; zeros from 16 KB0 up
        Wave w;
        for (int part = 0; part < 2; ++part)
            for (int kb = 0; kb < 2; ++kb)
                for (int e = 0; e < 2; ++e) {
                    std::vector<Access> acc;
                    for (int l = 0; l < WV; ++l) {
                        const int lj = l & 31, lh = l >> 5, c = 4 * kb + 2 * lh + e;
                        uint16_t v[4];
                        for (int i = 0; i < 4; ++i) v[i] = kb < KB0 ? value(part, lj, 4 * c + i) : 0;
                        const Access a = {l, TR_PART_BYTES * part + tr_chunk_offset(lj, c), 8};
                        w.store(a, v);
                        acc.push_back(a);
                    }
                    CHECK(ways(acc, 16, 32) <= 2, "8-byte store %d-way over its groups of sixteen lanes", ways(acc, 16, 32));
                    CHECK(ways(acc, 32, 64) <= 2, "8-byte store %d-way over a 32-lane half", ways(acc, 32, 64));
                }
        w.every_byte_once();
        check_reads(w, [KB0](int part, int s, int d) { return d < 16 * KB0 ? value(part, s, d) : (uint16_t)0; }, KB0 == 1 ? "inputs, KB0 = 1" : "inputs, KB0 = 2");
    }
    if (fails) { std::printf("%d checks failed\n", fails); return 1; }
    std::printf("ok\n");
    return 0;
}
'''


def _program():
    with open(os.path.join(CSRC, "policy_mfma.h")) as f:
        lines = [l for l in f if re.search(r"constexpr int frag_unit\(", l)]
    assert len(lines) == 1, "policy_mfma.h defines frag_unit in one line"
    return PROGRAM.replace("@FRAG_UNIT@", lines[0].replace("__host__ __device__", "").strip())


def test_image_maps_on_an_emulated_wavefront(tmp_path):
    src = tmp_path / "lds_tr_image_check.cpp"
    src.write_text(_program())
    exe = str(tmp_path / "lds_tr_image_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", exe])
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = res.stdout.decode()
    assert res.returncode == 0 and out.strip().endswith("ok"), out
