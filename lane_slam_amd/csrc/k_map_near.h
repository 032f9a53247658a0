// Association gated by the prior pose (k_map_near.hip, lanefront_map_near.hip): include/lanefront.h "lf_map_associate_near" is the
// contract, tests/map_near_ref.py its sequential restatement (a brute force over all rows).  Shared by the kernels and the host
// side; the cell function, the hash, the candidate test and the configurations' shared geometry also compile for the host
// (plain C++: define nothing, include <stdint.h> and include/lanefront.h first).
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#include "k_map_pairs.h"
#define LF_NR_HD __host__ __device__ inline
#else
#define LF_NR_HD inline
#endif

namespace lf {
namespace nr {

constexpr int kWg = 256;                   // rows per workgroup of the bin and fill kernels; lanes per workgroup of the query
constexpr int kGroup = 16;                 // lanes that share one segment in the query: 4 segments per wave
constexpr int kScanWg = 1024;              // lanes of the one workgroup that scans the buckets, four buckets per lane and turn
constexpr int kMinBuckets = kScanWg * 4;   // the table is a power of two of at least this, so a scan turn is never partial

// ---- the grid
// The walk visits the 3 x 3 cells around the segment's midpoint, so it is conservative when a candidate's midpoint is never more
// than one cell away per axis.  With cell == radius that fails: d2 <= r2 holds in rounded arithmetic for midpoints a few ulps more
// than `radius` apart, and the two quotients v / cell are rounded once more, so a passing entry can sit two cells away.  Hence
//     cell = max(radius (1 + 2^-10), 2^-490).
// From d2 <= r2 = fl(radius radius), with both squares in the normal range: |qmx - emx| <= radius (1 + 4 eps), eps = 2^-53 (one
// rounding each in r2, ddx ddx, the sum and ddx itself; a square so small that it is subnormal belongs to a |ddx| < 2^-511, which is
// far below any cell).  So the exact quotients differ by at most (1 + 6 eps) / (1 + 2^-10) < 1 - 2^-11.  Where one of them is at
// most 2^32 in magnitude the two roundings of the quotients add at most 2^-20, the rounded quotients differ by less than 1 and
// their floors by at most 1.  Where both are beyond 2^32 both floors are beyond the int32 range on the same side and clamp to the
// same cell.  The clamp is monotone and never widens a difference, so a pair with one floor inside the range and one beyond it
// stays within one cell too.  A radius below 2^-490 squares to less than 2^-980: then |ddx| < 2^-489, less than the floor of the
// cell's size, and the same argument holds with room to spare.  (A cell that overflows to +inf puts every midpoint into cell 0.)
LF_NR_HD double cell_size(double radius)
{
    const double c = radius * 1.0009765625, lo = 0x1p-490;
    return c > lo ? c : lo;
}

// floor(v / cell) clamped to int32; v is finite (a NaN quotient, which no caller makes, goes to cell 0)
LF_NR_HD int32_t cell_of(double v, double cell)
{
    const double a = v / cell;
    if (a >= 2147483647.0) return INT32_MAX;
    if (a <= -2147483648.0) return INT32_MIN;
    if (!(a == a)) return 0;
    const int32_t t = (int32_t)a;                  // truncates towards zero
    return (double)t > a ? t - 1 : t;              // the floor of a negative quotient that is no integer lies one below
}

// the bucket of a cell in a table of mask + 1 (a power of two) buckets
LF_NR_HD uint32_t bucket_of(int32_t cx, int32_t cy, uint32_t mask)
{
    uint32_t h = (uint32_t)cx * 0x9E3779B1u ^ (uint32_t)cy * 0x85EBCA77u;
    h ^= h >> 15; h *= 0x2C1B3C6Du; h ^= h >> 12;
    return h & mask;
}

LF_NR_HD bool finite_d(double v) { return v - v == 0.0; }      // false for NaN and the infinities

// an entry that can be a candidate at all: the contract's "entry t"
LF_NR_HD bool entry_valid(double ax, double ay, double bx, double by)
{
    if (!(finite_d(ax) && finite_d(ay) && finite_d(bx) && finite_d(by))) return false;
    const double ex = bx - ax, ey = by - ay;
    const double l2 = ex * ex + ey * ey;
    if (!(finite_d(l2) && l2 > 0.0)) return false;
    return finite_d((ax + bx) * 0.5) && finite_d((ay + by) * 0.5);      // a midpoint that overflows is infinitely far from every segment
}

// what the query kernel needs of a call, made once on the host
struct Rule {
    double r2, ms2, mo2, cell;             // radius radius, max_sin max_sin, max_offset max_offset, cell_size(radius)
    int test_sin, test_offset;             // max_sin < 1, max_offset finite
    int min_hits, gating, max_distance;    // the configuration's, the map's and the map's
};

// the reason a configuration's shared geometry is refused with, or null (lf_near_config's and lf_lanes_config's fields alike)
inline const char* bad_geometry(double radius, double max_offset, double max_sin, int min_hits)
{
    if (!finite_d(radius) || !(radius > 0)) return "radius is finite and > 0";
    if (!(max_offset > 0)) return "max_offset is > 0 or +inf";
    if (!(max_sin >= 0 && max_sin <= 1)) return "max_sin is 0 .. 1";
    if (min_hits < 0) return "min_hits is >= 0";
    return nullptr;
}

// the rule of a geometry that passed; gating and max_distance are 0: the map's, for the caller that reads them
inline Rule make_geometry(double radius, double max_offset, double max_sin, int min_hits)
{
    Rule c = {};
    c.r2 = radius * radius; c.ms2 = max_sin * max_sin; c.mo2 = max_offset * max_offset;
    c.cell = cell_size(radius);
    c.test_sin = max_sin < 1; c.test_offset = finite_d(max_offset) ? 1 : 0;
    c.min_hits = min_hits;
    return c;
}

// a segment in the map frame: the contract's "segment"
struct Seg { double sx, sy, S2, qmx, qmy; };

// the segment from a to b
LF_NR_HD Seg as_segment(double ax, double ay, double bx, double by)
{
    Seg s;
    s.sx = bx - ax; s.sy = by - ay;
    s.S2 = s.sx * s.sx + s.sy * s.sy;
    s.qmx = (ax + bx) * 0.5; s.qmy = (ay + by) * 0.5;
    return s;
}

// the contract's "candidate" but for hits and colour; d2 comes back for the winner's order
LF_NR_HD bool near_geometry(const Rule& c, const Seg& s, double ax, double ay, double bx, double by, double& d2)
{
    const double ex = bx - ax, ey = by - ay;
    const double l2 = ex * ex + ey * ey;
    const double emx = (ax + bx) * 0.5, emy = (ay + by) * 0.5;
    const double ddx = s.qmx - emx, ddy = s.qmy - emy;
    d2 = ddx * ddx + ddy * ddy;
    if (!(d2 <= c.r2)) return false;
    if (c.test_sin) {
        const double cr = s.sx * ey - s.sy * ex;
        if (!(cr * cr <= c.ms2 * (s.S2 * l2))) return false;
    }
    if (c.test_offset) {
        const double o = (s.qmx - ax) * ey - (s.qmy - ay) * ex;
        if (!(o * o <= c.mo2 * l2)) return false;
    }
    return true;
}

LF_NR_HD bool colours_agree(int a, int b) { return a == b || a >= 3 || b >= 3; }

#if defined(__HIPCC__)
// a valid row of the map in its bucket: 64 bytes, so a group of 16 lanes reads 1 KiB of consecutive records at a time
struct alignas(64) Rec {
    double ax, ay, bx, by;
    int32_t row, hits, colour, cx, cy;
    int32_t pad_[3];
};

// the index of one call: everything belongs to the map's handle
struct Index {
    int* start;                            // [buckets + 1]: counts, then their exclusive scan; start[buckets] = the valid rows
    int* cursor;                           // [buckets]: the next free slot of each bucket while the records are filled
    int* bucket;                           // [bound]: each row's bucket, -1: the row goes nowhere
    Rec* rec;                              // [bound]
    uint32_t mask;                         // buckets - 1
    int bound;                             // the host's upper bound of the map's size: sizes the grids and the arrays
};

// device arrays of one query
struct Query {
    const int* frame_offset; const uint8_t* code; const uint8_t* color; const double* ground;
    const double* pose4;                   // [n_frames][4] x, y, cos, sin
    int n, n_frames;
    int32_t* idx; float* dist; int32_t* n_near;      // n_near may be null
};

// the rows the kernels may touch: the map's size as the device knows it, never beyond what the host sized the arrays for
__device__ __forceinline__ int rows(const MapDevice& md, int bound)
{
    const int size = ma::map_size(md);
    return size < bound ? size : bound;
}

// The walk of the index, by a group of kLanes lanes of which this one is lane g: the 3 x 3 cells around (cx, cy), for each cell
// its bucket's records, the lanes striding over them, and f(rp, row, hits, colour) for every record OF THAT CELL.
// The index has two traps, and both are avoided here and nowhere else.  Double counting: a bucket holds other cells' rows, and
// two of the nine cells may share a bucket, so a bucket is visited FOR a cell and only that cell's records are looked at -- every
// entry is met exactly once.  The clamp: a neighbour beyond the int32 range is skipped (no midpoint has such a cell; wrapped
// round it would name the cell at the other end of the range), which takes the sum in 64 bits.
// row, hits, colour and cx are one 16-byte load, typed as the compiler's own vector so that it stays one once f is inlined (as an
// int4 it is taken apart into a load of cx and, behind the cell test, a second one of the rest: one more round trip per record).
template <int kLanes, class F>
__device__ __forceinline__ void for_each_near_record(const Index& ix, int32_t cx, int32_t cy, int g, F&& f)
{
    for (int dy = -1; dy <= 1; ++dy) {
        const long long wy = (long long)cy + dy;
        if (wy < INT32_MIN || wy > INT32_MAX) continue;
        for (int dx = -1; dx <= 1; ++dx) {
            const long long wx = (long long)cx + dx;
            if (wx < INT32_MIN || wx > INT32_MAX) continue;
            const uint32_t b = bucket_of((int32_t)wx, (int32_t)wy, ix.mask);
            const int end = ix.start[b + 1];
            for (int j = ix.start[b] + g; j < end; j += kLanes) {
                const Rec* rp = ix.rec + j;
                typedef int v4i __attribute__((ext_vector_type(4)));
                const v4i v = *reinterpret_cast<const v4i*>(&rp->row);
                if (v.w != (int32_t)wx || rp->cy != (int32_t)wy) continue;          // another cell's row in this bucket
                f(rp, v.x, v.y, v.z);
            }
        }
    }
}

// the buckets' counts (start[] is zero before), their scan, the records
void launch_near_index(const MapDevice& md, double cell, const Index& ix, hipStream_t s);
void launch_near_query(const Rule& c, const MapDevice& md, const Index& ix, const Query& q, hipStream_t s);
#endif

}  // namespace nr
}  // namespace lf
