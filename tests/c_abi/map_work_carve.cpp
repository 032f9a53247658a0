// ln::carve (k_map_lanes.h) and pl::carve (k_map_polylines.h), built as plain C++: for each "bound slots" given as arguments in
// pairs, both Work structs are carved once from no base (only the size) and once from a real buffer of exactly that size
// (malloc's, so 8-byte aligned).  Every array's element size and length below is the one the struct's own comment gives it ([bound], [bound][4], [bound][2],
// [slots], [slots][4]).  Checked: the two sizes agree, every array lies inside the buffer, no two overlap, the last one ends at
// the returned size, every 8-byte array is 8-byte aligned, and a sizing call hands out no pointer.  Every byte of every array is
// written, so a sanitizer build sees an array that leaves the buffer.  Prints one line per Work and pair; exit 1: a check failed.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "lanefront.h"
#include "k_map_polylines.h"

namespace {

struct Array { const char* name; const void* p; size_t elem, count; };

#define A(w, field, count) Array{ #field, (w).field, sizeof(*(w).field), (size_t)(count) }

std::vector<Array> arrays_of(const lf::ln::Work& w, size_t bound)
{
    return { A(w, parent, bound), A(w, root, bound), A(w, elig, bound), A(w, nl, bound), A(w, cnt, bound), A(w, lane_no, bound),
             A(w, hsum, bound), A(w, box, 4 * bound) };
}

std::vector<Array> arrays_of(const lf::pl::Work& w, size_t bound, size_t slots)
{
    return { A(w, part, bound), A(w, hx, bound), A(w, hy, bound), A(w, cx, bound), A(w, cy, bound), A(w, rslot, bound),
             A(w, own1, slots), A(w, own2, slots), A(w, cnt1, slots), A(w, sfirst, slots), A(w, sn, slots), A(w, svid, slots),
             A(w, shits, slots), A(w, ssum, 4 * slots),
             A(w, tmpv, bound), A(w, vslot, bound), A(w, fwd, bound), A(w, bwd, bound), A(w, nb, 2 * bound),
             A(w, parent, bound), A(w, root, bound), A(w, psize, bound), A(w, phead, bound), A(w, pn, bound),
             A(w, pid, bound), A(w, pfirst, bound), A(w, pos, bound), A(w, phits, bound) };
}

int fail(const char* what, const char* who, const char* name, size_t bound, size_t slots)
{
    fprintf(stderr, "%s: %s (%s) at bound %zu, slots %zu\n", who, what, name, bound, slots);
    return 1;
}

// the checks on one carving: `sized` arrays from the null base, `a` from `base`, which holds `bytes`
int check(const char* who, const std::vector<Array>& sized, std::vector<Array> a, char* base, size_t bytes, size_t from_null, size_t bound, size_t slots)
{
    if (from_null != bytes) return fail("the two sizes differ", who, "-", bound, slots);
    for (const Array& x : sized) if (x.p) return fail("a pointer from a null base", who, x.name, bound, slots);
    for (const Array& x : a) {
        const char* p = static_cast<const char*>(x.p);
        if (!p || p < base || p + x.elem * x.count > base + bytes) return fail("outside the buffer", who, x.name, bound, slots);
        if ((uintptr_t)p % x.elem && x.elem <= 8) return fail("not naturally aligned", who, x.name, bound, slots);
        if (x.elem >= 8 && (uintptr_t)p % 8) return fail("an 8-byte array that is not 8-byte aligned", who, x.name, bound, slots);
        memset(const_cast<char*>(p), 0x5A, x.elem * x.count);
    }
    std::sort(a.begin(), a.end(), [](const Array& l, const Array& r) { return l.p < r.p; });
    for (size_t k = 0; k + 1 < a.size(); ++k)
        if (static_cast<const char*>(a[k].p) + a[k].elem * a[k].count > static_cast<const char*>(a[k + 1].p)) return fail("overlaps the next array", who, a[k].name, bound, slots);
    const Array& last = a.back();
    if (static_cast<const char*>(last.p) + last.elem * last.count != base + bytes) return fail("the last array does not end at the returned size", who, last.name, bound, slots);
    printf("%s %zu %zu %zu %zu\n", who, bound, slots, bytes, a.size());
    return 0;
}

}  // namespace

int main(int argc, char** argv)
{
    for (int k = 1; k + 1 < argc; k += 2) {
        const size_t bound = strtoul(argv[k], nullptr, 10), slots = strtoul(argv[k + 1], nullptr, 10);
        {
            lf::ln::Work sized, w;
            memset(&sized, 0xFF, sizeof(sized)); memset(&w, 0, sizeof(w));
            const size_t from_null = lf::ln::carve(&sized, nullptr, bound);
            char* base = static_cast<char*>(malloc(from_null));                // (malloc: aligned for any scalar, so to 8 bytes)
            const size_t bytes = lf::ln::carve(&w, base, bound);
            const int rc = check("lanes", arrays_of(sized, bound), arrays_of(w, bound), base, bytes, from_null, bound, slots);
            free(base);
            if (rc) return rc;
        }
        {
            lf::pl::Work sized, w;
            memset(&sized, 0xFF, sizeof(sized)); memset(&w, 0, sizeof(w));
            const size_t from_null = lf::pl::carve(&sized, nullptr, bound, slots);
            char* base = static_cast<char*>(malloc(from_null));                // (malloc: aligned for any scalar, so to 8 bytes)
            const size_t bytes = lf::pl::carve(&w, base, bound, slots);
            const int rc = check("polylines", arrays_of(sized, bound, slots), arrays_of(w, bound, slots), base, bytes, from_null, bound, slots);
            free(base);
            if (rc) return rc;
        }
    }
    return 0;
}
