// Host-only check of the side-pruning bounds of csrc/vmas_physics.hpp (built and run by
// tests/test_side_prune_host.py).  On the host vote_all is the per-env predicate, so every sample
// decides for itself: stricter than the wave vote of the kernels.
//
// Per (family, class) one line:  <family> <class> samples=N mismatch=M all_pruned=A not3=K
//   mismatch   samples whose pruned closest points are not bitwise the unpruned ones
//   all_pruned samples in which some scan had all four sides pruned
//   not3       samples in which the pruned-side count is not exactly three (asserted for balance)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "vmas_physics.hpp"

using namespace vmas;

namespace {

struct Rng {
    uint64_t s;
    explicit Rng(uint64_t seed) : s(seed * 0x9E3779B97F4A7C15ull + 0x2545F4914F6CDD1Dull) {}
    uint64_t next() {
        s ^= s >> 12;
        s ^= s << 25;
        s ^= s >> 27;
        return s * 0x2545F4914F6CDD1Dull;
    }
    float u() { return (float)((next() >> 40) * (1.0 / 16777216.0)); }  // [0, 1)
    float in(float lo, float hi) { return lo + (hi - lo) * u(); }
    int below(int n) { return (int)(next() >> 33) % n; }
};

constexpr float kPi = 3.14159265358979f;

struct Case {
    V2 bpos;
    float brot, hl, hw;
    V2 tpos;          // sphere centre / line centre / second box centre
    float trot, thl;  // line or second box: rotation, half length
    float thw;        // second box: half width
};

// The kernels prune box-line pairs only (pair_bl_pruned = this scan + bl_finish); the same bounds
// are checked here on the box-sphere and box-box scans too (a point is a segment with a zero half
// vector; box-box runs the box-line scan per side).
V2 closest_point_box_pruned(V2 pos, Trig t, float hl, float hw, V2 tp) {
    const uint32_t pm = side_prune_mask(pos, t, hl, hw, tp, mk(0.f, 0.f));
    V2 best = mk(INFINITY, INFINITY);
    float bd = INFINITY;
    for (int i = 0; i < 4; ++i) {
        if ((pm >> i) & 1u) continue;
        const Seg s = box_side(pos, t, hl, hw, i);
        const V2 p = closest_point_line(s.p, s.dir, s.half, tp, true);
        const float d = norm(tp - p);
        if (d < bd) {
            bd = d;
            best = p;
        }
    }
    return best;
}
void closest_line_box_pruned(V2 bpos, Trig bt, float hl, float hw, Seg line, V2* pbox, V2* pline) {
    const Pts q = select_min_unpruned(4, line_prune_mask(bpos, bt, hl, hw, line), [&](int i) {
        Pts r;
        closest_points_line_line(box_side(bpos, bt, hl, hw, i), line, &r.p1, &r.p2);
        return r;
    });
    *pbox = q.p1;
    *pline = q.p2;
}
Pts bb_part_pruned(V2 pa, Trig ta, float hla, float hwa, V2 pb, Trig tb, float hlb, float hwb, int i) {
    Pts r;
    if (i < 4) closest_line_box_pruned(pb, tb, hlb, hwb, box_side(pa, ta, hla, hwa, i), &r.p2, &r.p1);
    else closest_line_box_pruned(pa, ta, hla, hwa, box_side(pb, tb, hlb, hwb, i - 4), &r.p1, &r.p2);
    return r;
}

bool same(const void* a, const void* b, size_t n) { return memcmp(a, b, n) == 0; }
int bits(uint32_t m) { return __builtin_popcount(m & 15u); }

struct Tally {
    long n = 0, mismatch = 0, all_pruned = 0, not3 = 0;
};

void check_bs(const Case& c, Tally& t) {
    const Trig bt = make_trig(c.brot);
    const V2 a = closest_point_box(c.bpos, bt, c.hl, c.hw, c.tpos);
    const V2 b = closest_point_box_pruned(c.bpos, bt, c.hl, c.hw, c.tpos);
    const uint32_t m = side_prune_mask(c.bpos, bt, c.hl, c.hw, c.tpos, mk(0.f, 0.f));
    ++t.n;
    t.mismatch += !same(&a, &b, sizeof a);
    t.all_pruned += bits(m) == 4;
    t.not3 += bits(m) != 3;
}

void check_bl(const Case& c, Tally& t) {
    const Trig bt = make_trig(c.brot);
    const Seg line{c.tpos, mk(cosf(c.trot), sinf(c.trot)), c.thl};
    V2 a[2], b[2];
    closest_line_box(c.bpos, bt, c.hl, c.hw, line, &a[0], &a[1]);
    closest_line_box_pruned(c.bpos, bt, c.hl, c.hw, line, &b[0], &b[1]);
    const uint32_t m = line_prune_mask(c.bpos, bt, c.hl, c.hw, line);
    // the pair as the kernels call it: force and torques too
    const WorldK wk{1e-3f, 100.f, 0.f, 0.f};
    const Trig lt{line.dir.x, line.dir.y, 0.f, 0.f};
    const PairOut fa = pair_bl(c.bpos, bt, c.hl, c.hw, false, c.tpos, lt, c.thl, kLineMinDist, wk);
    const PairOut fb = pair_bl_pruned(c.bpos, bt, c.hl, c.hw, false, c.tpos, lt, c.thl, kLineMinDist, wk);
    ++t.n;
    t.mismatch += !same(a, b, sizeof a) || !same(&fa, &fb, sizeof fa);
    t.all_pruned += bits(m) == 4;
    t.not3 += bits(m) != 3;
}

void check_bb(const Case& c, Tally& t) {
    const Trig ta = make_trig(c.brot), tb = make_trig(c.trot);
    V2 a[2];
    closest_box_box(c.bpos, ta, c.hl, c.hw, c.tpos, tb, c.thl, c.thw, &a[0], &a[1]);
    const Pts q = select_min(8, [&](int i) { return bb_part_pruned(c.bpos, ta, c.hl, c.hw, c.tpos, tb, c.thl, c.thw, i); });
    bool all = false, three = true;
    for (int i = 0; i < 8; ++i) {
        const uint32_t m = i < 4 ? line_prune_mask(c.tpos, tb, c.thl, c.thw, box_side(c.bpos, ta, c.hl, c.hw, i))
                                 : line_prune_mask(c.bpos, ta, c.hl, c.hw, box_side(c.tpos, tb, c.thl, c.thw, i - 4));
        all |= bits(m) == 4;
        three &= bits(m) == 3;
    }
    ++t.n;
    t.mismatch += !same(a, &q, sizeof a);
    t.all_pruned += all;
    t.not3 += !three;
}

// (a) balance: the floor 10 x 1 at (0, -1.53); the line (half length 0.4) anywhere the package
// can carry it, the spheres anywhere in the arena
Case balance(Rng& r, int cls) {
    Case c{mk(0.f, -1.53f), 0.f, 5.f, 0.5f, mk(0.f, 0.f), 0.f, 0.4f, 0.1f};
    if (cls == 0) c.tpos = mk(r.in(-1.5f, 1.5f), r.in(-1.f, 1.f));
    else c.tpos = mk(r.in(-1.4f, 1.4f), r.in(-1.03f, 1.f));
    c.trot = r.in(-kPi, kPi);
    return c;
}
// (b) small boxes, any rotation, targets within +-1.5
Case generic(Rng& r) {
    Case c;
    c.bpos = mk(r.in(-1.5f, 1.5f), r.in(-1.5f, 1.5f));
    c.brot = r.in(-kPi, kPi);
    c.hl = r.in(0.05f, 1.f);
    c.hw = r.in(0.05f, 1.f);
    c.tpos = mk(r.in(-1.5f, 1.5f), r.in(-1.5f, 1.5f));
    c.trot = r.in(-kPi, kPi);
    c.thl = r.in(0.05f, 1.f);
    c.thw = r.in(0.05f, 1.f);
    return c;
}
// (c) the target's centre inside the box (a long line or box then crosses its outline)
Case inside(Rng& r) {
    Case c = generic(r);
    const Trig t = make_trig(c.brot);
    const float x = r.in(-c.hl, c.hl), y = r.in(-c.hw, c.hw);
    c.tpos = mk(c.bpos.x + x * t.c0 + y * t.c1, c.bpos.y + x * t.s0 + y * t.s1);
    c.thl = r.in(0.01f, 2.f);
    return c;
}
// (d) family (b) scaled: the margin has to scale with the operands
Case scaled(Rng& r, float k) {
    Case c = generic(r);
    c.bpos = c.bpos * k;
    c.tpos = c.tpos * k;
    c.hl *= k;
    c.hw *= k;
    c.thl *= k;
    c.thw *= k;
    return c;
}
// (e) degenerate inputs on top of family (b) / (c)
Case degenerate(Rng& r, long i) {
    Case c = (i & 1) ? inside(r) : generic(r);
    const float bad[3] = {__builtin_nanf(""), INFINITY, -INFINITY};
    switch ((i >> 1) % 12) {
        case 0: c.thl = 0.f; break;                     // zero-length line / flat second box
        case 1: c.hw = 0.f; break;                      // zero half width
        case 2: c.hl = 0.f; break;
        case 3: c.hl = c.hw = 0.f; break;
        case 4: c.tpos.x = bad[r.below(3)]; break;
        case 5: c.tpos.y = bad[r.below(3)]; break;
        case 6: c.bpos.x = bad[r.below(3)]; break;
        case 7: c.bpos.y = bad[r.below(3)]; break;
        case 8: c.brot = bad[r.below(3)]; break;
        case 9: c.trot = bad[r.below(3)]; break;
        case 10: c.brot = r.in(-1.f, 1.f) * 1e6f; break;  // fl(rot + pi/2) skews the box frame
        default: c.tpos = c.bpos; c.thw = 0.f; break;    // coincident centres
    }
    return c;
}

}  // namespace

int main(int argc, char** argv) {
    const long n = argc > 1 ? atol(argv[1]) : 100000;
    const char* fam[] = {"a", "b", "c", "d3", "d4", "e"};
    const char* cls[] = {"bs", "bl", "bb"};
    for (int f = 0; f < 6; ++f)
        for (int k = 0; k < 3; ++k) {
            Rng r(1000u + 16u * f + k);
            Tally t;
            for (long i = 0; i < n; ++i) {
                const Case c = f == 0 ? balance(r, k) : f == 1 ? generic(r) : f == 2 ? inside(r)
                             : f == 3 ? scaled(r, 1e3f) : f == 4 ? scaled(r, 1e4f) : degenerate(r, i);
                if (k == 0) check_bs(c, t);
                else if (k == 1) check_bl(c, t);
                else check_bb(c, t);
            }
            printf("%s %s samples=%ld mismatch=%ld all_pruned=%ld not3=%ld\n", fam[f], cls[k], t.n, t.mismatch,
                   t.all_pruned, t.not3);
        }
    return 0;
}
