// The tiled line rasteriser of the live map's pictures, device side: what k_map_render.hip (the top-down view) and k_map_camera.hip
// (the map seen through the camera) share.  A line is the closed form of the midpoint line, so every step stands alone; a tile is
// kTile x kTile pixels whose winner -- the largest key -- is decided on a plane of 64-bit keys in LDS.  Nothing here depends on the
// order in which lanes arrive: a maximum has none.
#pragma once
#include "k_map_render.h"
#include "scan.h"

namespace lf {
namespace mr {

constexpr int kWg = 256;
constexpr double kPixLimit = 268435456.0;  // 2^28: coordinates of this magnitude and above are skipped

// a pixel's key: entries order by (last_seen, slot), last_seen as a biased u32 in bits 22..53, slot + 1 below it (capacity <= 2^21), so
// that no key is 0 = the background; a trajectory line has bit 62 and its index + 1
__device__ inline unsigned long long entry_key(int last_seen, unsigned slot)
{
    return ((unsigned long long)((unsigned)last_seen ^ 0x80000000u) << 22) | (unsigned long long)(slot + 1u);
}

// the three filters of a view; bit 3 of the mask stands for every colour value >= 3
__device__ inline bool selected(int min_hits, int min_last_seen, unsigned color_mask, int hits, int last_seen, unsigned color)
{
    return hits >= min_hits && last_seen >= min_last_seen && ((color_mask >> (color < 3u ? color : 3u)) & 1u);
}

// a line by its major (a) and minor (b) axis: pixel i = (a0 + i sa, b0 + sb floor((2 i m + n) / (2 n))), i = 0 .. n
struct Line {
    int a0, b0, sa, sb;
    long long n, m;
    bool xmajor;
};

__device__ inline Line make_line(const int4 p)
{
    const long long dx = (long long)p.z - p.x, dy = (long long)p.w - p.y;
    const long long ax = dx < 0 ? -dx : dx, ay = dy < 0 ? -dy : dy;
    const int sx = dx > 0 ? 1 : dx < 0 ? -1 : 0, sy = dy > 0 ? 1 : dy < 0 ? -1 : 0;
    Line L;
    L.xmajor = ax >= ay;
    if (L.xmajor) { L.a0 = p.x; L.b0 = p.y; L.sa = sx; L.sb = sy; L.n = ax; L.m = ay; }
    else { L.a0 = p.y; L.b0 = p.x; L.sa = sy; L.sb = sx; L.n = ay; L.m = ax; }
    return L;
}

__device__ inline long long minor_at(const Line& L, long long i)
{
    return L.n ? (long long)L.b0 + L.sb * ((2 * i * L.m + L.n) / (2 * L.n)) : (long long)L.b0;
}

// the steps i in [0, n] whose major coordinate lies in [lo, hi]; false: none
__device__ inline bool step_range(const Line& L, long long lo, long long hi, long long& ia, long long& ib)
{
    if (L.sa > 0) { ia = lo - L.a0; ib = hi - L.a0; }
    else if (L.sa < 0) { ia = L.a0 - hi; ib = L.a0 - lo; }
    else { ia = 0; ib = (L.a0 >= lo && L.a0 <= hi) ? 0 : -1; }
    if (ia < 0) ia = 0;
    if (ib > L.n) ib = L.n;
    return ia <= ib;
}

// The tiles a line's thickness-widened, image-clipped pixels fall into, one per next(): strip by strip along the major axis (a strip
// = the tiles of one tile column for an x-major line), and in a strip the tile range its minor coordinates span there -- the
// minor coordinate is monotonic in i and moves by at most 1 a step, so every tile between the two ends is crossed.
struct TileIter {
    Line L;
    int h0, h1, A, B, ntx;
    int ta, ta_end, cur, tb, tb_end;

    __device__ void init(const int4 p, int thickness, int rows, int cols, int ntx_)
    {
        L = make_line(p);
        h0 = (thickness - 1) / 2; h1 = thickness / 2;
        A = L.xmajor ? cols : rows; B = L.xmajor ? rows : cols; ntx = ntx_;
        long long e0 = L.a0, e1 = (long long)L.a0 + L.sa * L.n;
        if (e0 > e1) { const long long t = e0; e0 = e1; e1 = t; }
        e0 -= h0; e1 += h1;
        if (e0 < 0) e0 = 0;
        if (e1 > A - 1) e1 = A - 1;
        if (e0 > e1) { ta = 1; ta_end = 0; } else { ta = (int)(e0 / kTile); ta_end = (int)(e1 / kTile); }
        cur = 0; tb = 1; tb_end = 0;
    }
    __device__ bool next(unsigned& tile)
    {
        while (tb > tb_end) {
            if (ta > ta_end) return false;
            const long long lo = (long long)ta * kTile, hi = lo + kTile - 1 < A - 1 ? lo + kTile - 1 : A - 1;
            long long ia, ib;
            if (step_range(L, lo - h1, hi + h0, ia, ib)) {
                long long ba = minor_at(L, ia), bb = minor_at(L, ib);
                if (ba > bb) { const long long t = ba; ba = bb; bb = t; }
                ba -= h0; bb += h1;
                if (ba < 0) ba = 0;
                if (bb > B - 1) bb = B - 1;
                if (ba <= bb) { tb = (int)(ba / kTile); tb_end = (int)(bb / kTile); }
            }
            cur = ta++;
        }
        tile = L.xmajor ? (unsigned)(tb * ntx + cur) : (unsigned)(cur * ntx + tb);
        ++tb;
        return true;
    }
};

// ctr[t] += 1 for every active lane, one atomic per distinct t of the wave (a map built while the robot stands still sends a whole
// wave to one tile); returns the lane's own position.  Called by all lanes of a wave together.
__device__ inline unsigned wave_add(unsigned* ctr, unsigned t, bool active, int lane)
{
    unsigned pos = 0;
    unsigned long long todo = __ballot(active);
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const unsigned t0 = (unsigned)__shfl((int)t, leader);
        const bool mine = active && t == t0;
        const unsigned long long same = __ballot(mine);
        unsigned base = 0;
        if (lane == leader) base = atomicAdd(&ctr[t0], (unsigned)__popcll(same));
        base = (unsigned)__shfl((int)base, leader);
        if (mine) pos = base + lanes_below(same, lane);
        todo &= ~same;
    }
    return pos;
}

// The winners of one tile, columns c0 .. c1 and rows r0 .. r1 of the image, on `plane` (kTile x kTile keys, zeroed, in LDS), by a
// workgroup of kWg lanes that all call this together: record(k, p, key) gives the pixel endpoints and the key of the tile's k-th
// line, k < n_rec.  64 records a wave at a time; their (line, step) pairs are dealt to the lanes in order, so that a long line among
// short ones keeps no lane waiting: pair `item` belongs to the first record whose inclusive step count exceeds it.  The caller
// synchronises the workgroup before it reads the plane.
template <typename Record>
__device__ inline void paint_records(unsigned long long* plane, unsigned n_rec, int c0, int c1, int r0, int r1, int h0, int h1, Record record)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (unsigned base = (unsigned)wave * 64u; base < n_rec; base += kWg) {
        int4 p = make_int4(0, 0, 0, 0);
        unsigned long long key = 0ull;
        int cnt = 0, i0 = 0;
        if (base + lane < n_rec) {
            record(base + lane, p, key);
            const Line L = make_line(p);
            long long ia, ib;
            if (step_range(L, (long long)(L.xmajor ? c0 : r0) - h1, (long long)(L.xmajor ? c1 : r1) + h0, ia, ib)) { cnt = (int)(ib - ia + 1); i0 = (int)ia; }
        }
        const int inc = wave_incl_scan(cnt, lane);
        const int total = __shfl(inc, 63);
        for (int first = 0; first < total; first += 64) {
            const int item = first + lane;
            int lo = 0, hi = 63;
            for (int s = 0; s < 6; ++s) {
                const int mid = (lo + hi) >> 1;
                if (__shfl(inc, mid) > item) hi = mid; else lo = mid + 1;
            }
            const int j = lo < 63 ? lo : 63;
            const int excl = __shfl(inc - cnt, j), ji0 = __shfl(i0, j);
            const int4 jp = make_int4(__shfl(p.x, j), __shfl(p.y, j), __shfl(p.z, j), __shfl(p.w, j));
            const unsigned klo = (unsigned)__shfl((int)(unsigned)(key & 0xffffffffull), j), khi = (unsigned)__shfl((int)(unsigned)(key >> 32), j);
            if (item < total) {
                const unsigned long long jkey = ((unsigned long long)khi << 32) | klo;
                const Line L = make_line(jp);
                const long long i = (long long)ji0 + (item - excl);
                const long long a = (long long)L.a0 + L.sa * i, b = minor_at(L, i);
                const int u = (int)(L.xmajor ? a : b), w = (int)(L.xmajor ? b : a);
                const int ca = u - h0 > c0 ? u - h0 : c0, cb = u + h1 < c1 ? u + h1 : c1;
                const int ra = w - h0 > r0 ? w - h0 : r0, rb = w + h1 < r1 ? w + h1 : r1;
                for (int rr = ra; rr <= rb; ++rr)
                    for (int cc = ca; cc <= cb; ++cc) {
                        unsigned long long* q = &plane[(rr - r0) * kTile + (cc - c0)];
                        if (*q < jkey) atomicMax(q, jkey);       // (the read only spares atomics: keys never go down)
                    }
            }
        }
    }
}

// Rows r0 .. r1, columns c0 .. c1 of the BGR image at `image` ([..][cols][3]), one tile's, written by a workgroup of kWg lanes that
// all call this together.  A tile row is up to 192 bytes and starts at any address: a lane takes the aligned dword it lies in and
// writes it whole when all four bytes are to be stored, byte by byte otherwise -- at the two ends of the row, so that no byte
// outside the tile's own is touched, and wherever byte() leaves one out.  byte(r, pix, ch, off, b): the value b of channel ch of the
// tile's pixel (row r, column pix), off = 3 pix + ch its offset in the tile row; false: the byte stays as it is.
template <typename Byte>
__device__ inline void store_tile_rows(uint8_t* image, int cols, int c0, int c1, int r0, int r1, Byte byte)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int nbytes = (c1 - c0 + 1) * 3;
    for (int r = wave; r0 + r <= r1; r += kWg / 64) {
        const uintptr_t a0 = reinterpret_cast<uintptr_t>(image) + ((size_t)(r0 + r) * cols + c0) * 3;
        const uintptr_t word = (a0 & ~(uintptr_t)3) + 4u * (unsigned)lane;
        unsigned val = 0, todo = 0;
        for (int k = 0; k < 4; ++k) {
            const long long off = (long long)(word + k) - (long long)a0;
            if (off >= 0 && off < nbytes) {
                const int pix = (int)off / 3, ch = (int)off - 3 * pix;
                unsigned b = 0;
                if (byte(r, pix, ch, (int)off, b)) { val |= (b & 255u) << (8 * k); todo |= 1u << k; }
            }
        }
        if (todo == 15u) *reinterpret_cast<unsigned*>(word) = val;
        else
            for (int k = 0; k < 4; ++k) if ((todo >> k) & 1u) *reinterpret_cast<uint8_t*>(word + k) = (uint8_t)(val >> (8 * k));
    }
}

}  // namespace mr
}  // namespace lf
