// Which bytes a launch reads and writes, and whether they may alias: the one definition every host launcher uses (DESIGN.md:
// "One definition: memory ranges").  Plain C++: no HIP, no state.
//
// A range here is what can ALIAS: from the first byte an access can touch to one past the last.  It is not the extent a kernel's
// buffer resource is given (what the hardware clamps), which may reach further: those stay with the launchers.
#pragma once
#include <stdint.h>
#include <initializer_list>

// [p, p + bytes); p == nullptr or bytes <= 0: empty, overlaps nothing
struct ml_range {
    const void *p;
    long long bytes;
};

// the two ranges share a byte
inline bool ml_ranges_overlap(const void *a, long long abytes, const void *b, long long bbytes) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return a && b && abytes > 0 && bbytes > 0 && pa < pb + (uintptr_t)bbytes && pb < pa + (uintptr_t)abytes;
}

// some a[i] shares a byte with some b[j]
inline bool ml_any_overlap(const ml_range *a, int na, const ml_range *b, int nb) {
    for (int i = 0; i < na; ++i)
        for (int j = 0; j < nb; ++j)
            if (ml_ranges_overlap(a[i].p, a[i].bytes, b[j].p, b[j].bytes)) return true;
    return false;
}
inline bool ml_any_overlap(std::initializer_list<ml_range> a, std::initializer_list<ml_range> b) {
    return ml_any_overlap(a.begin(), (int)a.size(), b.begin(), (int)b.size());
}

// out = in + something, element by element, is safe: there is no `in`, or it is `out` itself (an element is read before it is
// written), or the two are apart.  A shifted view is refused.
inline bool ml_add_or_disjoint(const void *out, const void *in, long long bytes) {
    return in == out || !ml_ranges_overlap(out, bytes, in, bytes);
}

// Elements from the first element of a strided NHWC view to one past its last: B images `bstride` apart (0: dense, P * cstride),
// P pixels `cstride` apart, C channels each.  The last pixel ends after its C channels, not after a whole cstride: a channel
// slice of a concat tensor ends inside that tensor.
inline long long ml_view_elems(long long B, long long bstride, long long P, long long cstride, long long C) {
    return (B - 1) * (bstride ? bstride : P * cstride) + (P - 1) * cstride + C;
}
