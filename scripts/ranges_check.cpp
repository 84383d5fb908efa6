// Stand-alone host check of csrc/ranges.h: c++ -std=c++17 -fsanitize=address,undefined -I<csrc> ranges_check.cpp && ./a.out
// Empty ranges, null pointers, abutting and one-byte overlaps; ml_any_overlap against the pairwise loop on pseudo-random ranges;
// ml_view_elems against the largest index a view's loops reach.  Prints one line; exit status 0 means every check held.
#include "ranges.h"
#include <stdio.h>

static int fails = 0;
#define CHECK(c) do { if (!(c)) { ++fails; printf("line %d: %s\n", __LINE__, #c); } } while (0)

int main() {
    static char buf[4096];
    CHECK(!ml_ranges_overlap(buf, 0, buf, 8) && !ml_ranges_overlap(buf + 4, -1, buf, 8) && !ml_ranges_overlap(buf, 8, buf + 4, 0));
    CHECK(!ml_ranges_overlap(nullptr, 8, buf, 8) && !ml_ranges_overlap(buf, 8, nullptr, 8) && !ml_ranges_overlap(nullptr, 8, nullptr, 8));
    CHECK(!ml_ranges_overlap(buf, 8, buf + 8, 8) && !ml_ranges_overlap(buf + 8, 8, buf, 8));            // abutting
    CHECK(ml_ranges_overlap(buf, 9, buf + 8, 8) && ml_ranges_overlap(buf + 8, 8, buf, 9));              // one byte
    CHECK(ml_ranges_overlap(buf, 64, buf + 8, 1) && ml_ranges_overlap(buf, 8, buf, 8));                 // inside, equal
    CHECK(ml_add_or_disjoint(buf, nullptr, 8) && ml_add_or_disjoint(buf, buf, 8) && ml_add_or_disjoint(buf, buf + 8, 8));
    CHECK(!ml_add_or_disjoint(buf, buf + 7, 8) && !ml_add_or_disjoint(buf + 7, buf, 8));
    CHECK(!ml_any_overlap({}, {{buf, 8}}) && !ml_any_overlap({{buf, 8}}, {}) && !ml_any_overlap({{nullptr, 8}, {buf, 0}}, {{buf, 8}}));
    unsigned s = 12345;
    auto rnd = [&](unsigned n) { s = s * 1664525u + 1013904223u; return (s >> 8) % n; };
    int hits = 0;
    for (int t = 0; t < 400; ++t) {
        ml_range a[3], b[4];
        for (ml_range &r : a) r = {rnd(8) ? buf + rnd(300) : nullptr, (long long)rnd(40) - 4};
        for (ml_range &r : b) r = {rnd(8) ? buf + rnd(300) : nullptr, (long long)rnd(40) - 4};
        bool want = false;
        for (const ml_range &x : a)
            for (const ml_range &y : b)
                for (long long i = 0; x.p && y.p && i < x.bytes; ++i)                                  // byte by byte
                    want |= (const char *)x.p + i >= (const char *)y.p && (const char *)x.p + i < (const char *)y.p + y.bytes;
        CHECK(ml_any_overlap(a, 3, b, 4) == want && ml_any_overlap({a[0], a[1], a[2]}, {b[0], b[1], b[2], b[3]}) == want);
        hits += want;
    }
    CHECK(hits > 40 && hits < 360);
    int views = 0;
    for (long long B = 1; B <= 3; ++B)
        for (long long P = 1; P <= 4; ++P)
            for (long long Cn = 1; Cn <= 5; ++Cn)
                for (long long cs = Cn; cs <= Cn + 3; ++cs)
                    for (long long bs : {0ll, P * cs, P * cs + 7}) {
                        long long last = -1;
                        for (long long b = 0; b < B; ++b)
                            for (long long p = 0; p < P; ++p)
                                for (long long c = 0; c < Cn; ++c) {
                                    const long long i = b * (bs ? bs : P * cs) + p * cs + c;
                                    last = i > last ? i : last;
                                }
                        CHECK(ml_view_elems(B, bs, P, cs, Cn) == last + 1);
                        ++views;
                    }
    printf("ranges_check: %s (400 random range sets, %d overlapping; %d views)\n", fails ? "FAILED" : "ok", hits, views);
    return fails != 0;
}
