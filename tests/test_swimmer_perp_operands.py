"""`substep_quad` (dyn_swimmer_chain.h) holds no perpendicular `Ap = (-sn, cs)` and no `Gp = Ap * db`: every product with
them reads `A` / `G` through a swizzle, the sign on one half of one operand.  A stand-alone C++ program (the oracle
build's compiler and flags: per-expression contraction, hardware FMA) includes the header and checks on the host:

* the lock-step emulation of the four lanes against `substep_scalar`, bit for bit, in float and double, 50 sub-steps
  from chain states given DIRECTLY (not through `to_chain`, whose sines and cosines never are a negative zero): body
  directions with sn = +0, sn = -0 and cs = -0, a chain at rest under zero and negative-zero torques (every angular
  acceleration thb is a signed zero), each hinge beyond each of its limits, random moving states; the zero lane's
  db = 0 takes part in every one of them;
* `perp_mul(G, t)` (what the sub-step computes now) against `(Ap * db) * t` (what it computed) under memcmp, for 10^4
  random and every pair of special values (signed zeros, infinities, the smallest and largest finite numbers).
"""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rllab_amd", "csrc")

PROGRAM = r'''
#include <array>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>
#include "dyn_swimmer.h"

using Chain = rl::Swimmer::Chain;
static int fails = 0;

// one pass per exchange point: pass k answers the first k points from the log of earlier passes and records point k
template <typename R>
struct Replay {
    int lane, filled, counter;
    std::vector<std::array<R, 4>>* log;
    template <int CTRL> R qp(R v) {
        const int k = counter++;
        if (k < filled) return (*log)[k][(CTRL >> (2 * lane)) & 3];
        if ((int)log->size() <= k) log->resize(k + 1);
        if (k == filled) (*log)[k][lane] = v;
        return v;
    }
};

template <typename R>
struct State { R r[4], cs[3], sn[3], om[3], th[3], act[3]; };

template <typename R>
static bool same(R a, R b) { return std::memcmp(&a, &b, sizeof(R)) == 0; }

template <typename R>
static void compare(const State<R>& s0, int nsub, const char* what, int id) {
    const R h = (R)0.001;
    State<R> s = s0;
    for (int it = 0; it < nsub; ++it) Chain::template substep_scalar<R>(s.r, s.cs, s.sn, s.om, s.th, s.act, h);
    Chain::Lane<R> lanes[4];
    Chain::LaneConst<R> consts[4];
    for (int b = 0; b < 4; ++b) {
        consts[b] = Chain::template lane_const<R>(b);
        lanes[b].set_direction(b < 3 ? s0.cs[b] : (R)1, b < 3 ? s0.sn[b] : (R)0);
        lanes[b].om = b < 3 ? s0.om[b] : (R)0;
        lanes[b].th = b < 3 ? s0.th[b] : (R)0;
        lanes[b].r = rl::V2<R>{s0.r[0], s0.r[1]};
        lanes[b].v = rl::V2<R>{s0.r[2], s0.r[3]};
    }
    for (int b = 0; b < 4; ++b) lanes[b].qd = lanes[b].om - lanes[(b + 3) & 3].om;
    for (int it = 0; it < nsub; ++it) {
        std::vector<std::array<R, 4>> log;
        int n_points = -1;
        Chain::Lane<R> result[4];
        for (int pass = 0; n_points < 0 || pass <= n_points; ++pass)
            for (int b = 0; b < 4; ++b) {
                Replay<R> x{b, pass, 0, &log};
                Chain::Lane<R> l = lanes[b];
                Chain::template substep_quad<R>(x, consts[b], l, b < 3 ? s0.act[b] : (R)0, h);
                n_points = x.counter;
                result[b] = l;
            }
        for (int b = 0; b < 4; ++b) lanes[b] = result[b];
    }
    bool ok = same(lanes[3].om, (R)0);
    for (int b = 0; b < 4; ++b)
        ok = ok && same(lanes[b].r.x, s.r[0]) && same(lanes[b].r.y, s.r[1]) && same(lanes[b].v.x, s.r[2]) &&
             same(lanes[b].v.y, s.r[3]);
    for (int b = 0; b < 3; ++b)
        ok = ok && same(lanes[b].A.x, s.cs[b]) && same(lanes[b].A.y, s.sn[b]) && same(lanes[b].om, s.om[b]) &&
             same(lanes[b].th, s.th[b]) && same(lanes[b].qd, b == 0 ? s.om[0] : s.om[b] - s.om[b - 1]);
    bool finite = true;
    for (int b = 0; b < 3; ++b) finite = finite && s.om[b] - s.om[b] == (R)0 && s.cs[b] - s.cs[b] == (R)0;
    if (!ok || !finite) {
        ++fails;
        std::printf("%s state %d (%s): %s\n", what, id, sizeof(R) == 4 ? "float" : "double", ok ? "not finite" : "DIFFERENT");
    }
}

static uint64_t lcg = 0x9E3779B97F4A7C15ull;
static double uni() { lcg = lcg * 6364136223846793005ull + 1442695040888963407ull; return (double)(lcg >> 11) / 9007199254740992.0; }
static double sym(double a) { return a * (2.0 * uni() - 1.0); }

template <typename R>
static int chain_cases() {
    int n = 0;
    const R Z = (R)0, NZ = -(R)0, ONE = (R)1;
    // (cs, sn) with a zero component of either sign; cs = -0 goes with sn = +-1
    const R dirs[6][2] = {{ONE, Z}, {ONE, NZ}, {-ONE, Z}, {-ONE, NZ}, {NZ, ONE}, {NZ, -ONE}};
    const R lim = (R)1.9;     // beyond the hinge range of +-100 degrees
    for (int moving = 0; moving < 2; ++moving)
        for (int d0 = 0; d0 < 6; ++d0)
            for (int d1 = 0; d1 < 6; ++d1) {
                // at rest (every thb is a signed zero, of either sign under +0 / -0 torques) and moving
                State<R> s{};
                const int d2 = (d0 + 2 * d1 + 1) % 6;
                const int d[3] = {d0, d1, d2};
                for (int b = 0; b < 3; ++b) { s.cs[b] = dirs[d[b]][0]; s.sn[b] = dirs[d[b]][1]; }
                s.r[0] = (R)0.1; s.r[1] = (R)-0.2;
                s.act[1] = (d0 & 1) ? NZ : Z; s.act[2] = (d1 & 1) ? NZ : Z;
                s.th[0] = (R)0.3;
                if (moving) {
                    s.r[2] = (R)sym(1.0); s.r[3] = (R)sym(1.0);
                    for (int b = 0; b < 3; ++b) s.om[b] = (R)sym(3.0);
                    s.act[1] = (R)sym(1.0); s.act[2] = (R)sym(1.0);
                    s.th[1] = (R)sym(1.0); s.th[2] = (R)sym(1.0);
                } else if (d2 & 1) {
                    for (int b = 0; b < 3; ++b) s.om[b] = NZ;
                    s.r[2] = NZ; s.r[3] = NZ;
                }
                compare<R>(s, 50, moving ? "zero-component direction, moving" : "zero-component direction, at rest", n++);
            }
    // each hinge beyond each limit (the carried (cs, sn) only have to be unit vectors: they are state of their own)
    for (int k = 0; k < 16; ++k) {
        State<R> s{};
        for (int b = 0; b < 3; ++b) {
            const double phi = sym(3.1);
            s.cs[b] = (R)__builtin_cos(phi); s.sn[b] = (R)__builtin_sin(phi);
            s.om[b] = (k & 8) ? (R)sym(3.0) : Z;
        }
        s.th[0] = (R)sym(3.0);
        s.th[1] = (k & 1) ? lim : ((k & 2) ? -lim : (R)sym(1.0));
        s.th[2] = (k & 4) ? ((k & 1) ? -lim : lim) : (R)sym(1.0);
        if (k == 0) s.th[2] = -lim;
        s.act[1] = (R)sym(1.0); s.act[2] = (R)sym(1.0);
        s.r[2] = (R)sym(1.0); s.r[3] = (R)sym(1.0);
        compare<R>(s, 50, "hinge beyond a limit", n++);
    }
    for (int k = 0; k < 24; ++k) {
        State<R> s{};
        for (int b = 0; b < 3; ++b) {
            const double phi = sym(3.1);
            s.cs[b] = (R)__builtin_cos(phi); s.sn[b] = (R)__builtin_sin(phi);
            s.om[b] = (R)sym(4.0);
            s.th[b] = (R)sym(1.6);
        }
        for (int i = 0; i < 4; ++i) s.r[i] = (R)sym(1.0);
        s.act[1] = (R)sym(1.0); s.act[2] = (R)sym(1.0);
        compare<R>(s, 50, "random", n++);
    }
    return n;
}

// what the sub-step computes now against what it computed: cp = (Ap * db) * t with Ap = (-sn, cs)
template <typename R>
static int product_cases() {
    using P = rl::V2<R>;
    const R inf = std::numeric_limits<R>::infinity(), big = std::numeric_limits<R>::max(),
            tiny = std::numeric_limits<R>::denorm_min(), nrm = std::numeric_limits<R>::min();
    const R special[] = {(R)0, -(R)0, inf, -inf, big, -big, tiny, -tiny, nrm, -nrm, (R)1, -(R)1};
    const int NS = sizeof(special) / sizeof(special[0]);
    int n = 0;
    auto check = [&](R cs, R sn, R db, R t) {
        const P A = P{cs, sn}, Ap = P{-sn, cs};
        const P G = A * db;
        const P Gp = Ap * db;
        const P was = Gp * t;
        const P now = Chain::perp_mul(G, t);
        // a NaN (0 * inf) carries no sign that anything reads: both must be one
        const bool bx = (was.x != was.x) ? (now.x != now.x) : same(was.x, now.x);
        const bool by = (was.y != was.y) ? (now.y != now.y) : same(was.y, now.y);
        if (!(bx && by)) {
            ++fails;
            std::printf("product (%s): cs %a sn %a db %a t %a: was (%a, %a) now (%a, %a)\n", sizeof(R) == 4 ? "float" : "double",
                        (double)cs, (double)sn, (double)db, (double)t, (double)was.x, (double)was.y, (double)now.x, (double)now.y);
        }
        ++n;
    };
    for (int i = 0; i < NS; ++i)
        for (int j = 0; j < NS; ++j)
            for (int k = 0; k < NS; ++k) {
                check(special[i], special[j], special[k], (R)sym(2.0));
                check(special[i], (R)sym(1.0), special[j], special[k]);
                check((R)sym(1.0), special[i], special[j], special[k]);
            }
    for (int b = 0; b < 4; ++b) {           // the lanes' own db, the zero lane's 0 among them
        const R db = Chain::template lane_const<R>(b).db;
        for (int i = 0; i < NS; ++i) { check((R)sym(1.0), (R)sym(1.0), db, special[i]); check(special[i], (R)sym(1.0), db, (R)sym(50.0)); }
    }
    for (int i = 0; i < 10000; ++i) {
        const double phi = sym(3.2), scale = __builtin_exp(sym(40.0));
        check((R)__builtin_cos(phi), (R)__builtin_sin(phi), (R)sym(2.0), (R)(sym(1.0) * scale));
    }
    return n;
}

int main() {
    const int nf = chain_cases<float>(), nd = chain_cases<double>();
    const int pf = product_cases<float>(), pd = product_cases<double>();
    std::printf("chain states: %d float, %d double; products: %d float, %d double\n", nf, nd, pf, pd);
    if (fails) { std::printf("%d checks failed\n", fails); return 1; }
    std::printf("ok\n");
    return 0;
}
'''


def _oracle_compiler():
    """the compiler and the flags of the host oracle build (oracle/Makefile): the same front-end as the device build,
    contraction per expression, hardware fused multiply-add"""
    with open(os.path.join(ROOT, "oracle", "Makefile")) as f:
        mk = f.read()
    cxx = re.search(r"^CXX\s*=\s*(\S+)", mk, re.M).group(1)
    flags = re.search(r"^CXXFLAGS\s*=\s*(.+)$", mk, re.M).group(1).split()
    assert "-ffp-contract=on" in flags and "-mfma" in flags
    return cxx, [f for f in flags if f != "-fPIC"]


def test_lane_program_without_the_perpendicular_is_bitwise_the_scalar_program(tmp_path):
    cxx, flags = _oracle_compiler()
    src = tmp_path / "swimmer_perp_check.cpp"
    src.write_text(PROGRAM)
    exe = str(tmp_path / "swimmer_perp_check")
    subprocess.check_call([cxx] + flags + ["-I", CSRC, str(src), "-o", exe])
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = res.stdout.decode()
    print(out)
    assert res.returncode == 0 and out.strip().endswith("ok"), out
    m = re.search(r"chain states: (\d+) float, (\d+) double; products: (\d+) float, (\d+) double", out)
    assert m and int(m.group(1)) == int(m.group(2)) >= 100 and min(int(m.group(3)), int(m.group(4))) >= 10000
