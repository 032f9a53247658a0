// lf_map_render / lf_map_bounds: the live map (k_map.hip) rasterised into a top-down BGR image, the reference's RViz view of
// show_map's LINE_LIST markers (src/show_map/src/show_map.py:44-72) and odometry's LINE_STRIP (src/odometry/src/odometry.py:50-62).
// The pixel contract is the package's own (include/lanefront.h "lf_map_render"; tests/map_render_ref.py restates it sequentially):
//   pixel of a point   u = floor((X - x_min) * ppm), v = floor((y_max - Y) * ppm), f64, unfused (this file is built -ffp-contract=off)
//   pixels of a line   the closed form of the midpoint line: step i of the major axis alone gives the minor coordinate, so any lane
//                      may start anywhere on a line and clipping is a restriction of i
//   the winner         the largest (last_seen, slot) among the entries that paint a pixel; trajectory lines above all, later ones first
// Tiles of 64 x 64 pixels with the winner decided in LDS: 1 project (pixel endpoints, the skip rule, per-tile counts), 2 scan,
// 3 bin (the lines of every tile, by the tiles a line CROSSES, not by its bounding box), 4 paint (one workgroup per tile: 64-bit
// atomic max of the keys on an LDS plane, then the colours, written as whole dwords).  Nothing depends on the order in which lanes
// arrive: a maximum has none.
#include "k_map_render.h"

namespace lf {
namespace mr {

namespace {

constexpr int kWg = 256;
constexpr unsigned long long kTrajBit = 1ull << 62;
constexpr double kPixLimit = 268435456.0;      // 2^28: coordinates of this magnitude and above are skipped

// a pixel's key: entries order by (last_seen, slot), last_seen as a biased u32 in bits 22..53, slot + 1 below it (capacity <= 2^21), so
// that no key is 0 = the background; a trajectory line has bit 62 and its index + 1
__device__ inline unsigned long long entry_key(int last_seen, unsigned slot)
{
    return ((unsigned long long)((unsigned)last_seen ^ 0x80000000u) << 22) | (unsigned long long)(slot + 1u);
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

    __device__ void init(const int4 p, const View& v)
    {
        L = make_line(p);
        h0 = (v.thickness - 1) / 2; h1 = v.thickness / 2;
        A = L.xmajor ? v.cols : v.rows; B = L.xmajor ? v.rows : v.cols; ntx = v.ntx;
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
        if (mine) pos = base + (unsigned)__popcll(same & ((1ull << lane) - 1ull));
        todo &= ~same;
    }
    return pos;
}

__device__ inline bool selected(const View& v, int hits, int last_seen, unsigned color)
{
    return hits >= v.min_hits && last_seen >= v.min_last_seen && ((v.color_mask >> (color < 3u ? color : 3u)) & 1u);
}

__global__ void __launch_bounds__(kWg) k_mr_project(const View v, const int capacity, const int* __restrict__ state,
                                                    const uint8_t* __restrict__ color, const double* __restrict__ ground,
                                                    const int* __restrict__ hits, const int* __restrict__ last_seen,
                                                    const double* __restrict__ traj, const long long n_traj, int4* __restrict__ px,
                                                    unsigned* __restrict__ tile_count, int* __restrict__ counters)
{
    const long long i = (long long)blockIdx.x * kWg + threadIdx.x;
    const int lane = threadIdx.x & 63;
    bool have = false;
    double g[4] = { 0, 0, 0, 0 };
    if (i < capacity) {
        if (i < state[0] && selected(v, hits[i], last_seen[i], color[i])) {
            have = true;
            for (int k = 0; k < 4; ++k) g[k] = ground[(size_t)i * 4 + k];
        }
    } else if (i - capacity < n_traj) {
        have = true;
        for (int k = 0; k < 4; ++k) g[k] = traj[(size_t)(i - capacity) * 2 + k];
    }
    bool drawn = false;
    int4 p = make_int4(kNotDrawn, 0, 0, 0);
    if (have) {
        const double f[4] = { floor((g[0] - v.x_min) * v.ppm), floor((v.y_max - g[1]) * v.ppm),
                              floor((g[2] - v.x_min) * v.ppm), floor((v.y_max - g[3]) * v.ppm) };
        drawn = fabs(f[0]) < kPixLimit && fabs(f[1]) < kPixLimit && fabs(f[2]) < kPixLimit && fabs(f[3]) < kPixLimit;   // (false for a NaN)
        if (drawn) p = make_int4((int)f[0], (int)f[1], (int)f[2], (int)f[3]);
    }
    if (i < capacity + n_traj) px[i] = p;
    const unsigned long long bd = __ballot(drawn), bs = __ballot(have && !drawn);
    if (lane == 0) {
        if (bd) atomicAdd(&counters[0], (int)__popcll(bd));
        if (bs) atomicAdd(&counters[1], (int)__popcll(bs));
    }
    TileIter it;
    if (drawn) it.init(p, v);
    bool more = drawn;
    unsigned tile = 0;
    for (;;) {
        if (more) more = it.next(tile);
        if (!__any(more)) break;
        wave_add(tile_count, tile, more, lane);
    }
}

__global__ void __launch_bounds__(1024) k_mr_scan(const int n_tiles, const unsigned* __restrict__ tile_count, unsigned* __restrict__ tile_start,
                                                  unsigned* __restrict__ cursor, int* __restrict__ counters)
{
    __shared__ unsigned long long s_sum[1024];
    const int t = threadIdx.x, per = (n_tiles + 1023) / 1024, a = t * per;
    unsigned long long sum = 0;
    for (int k = 0; k < per; ++k) if (a + k < n_tiles) sum += tile_count[a + k];
    s_sum[t] = sum;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        const unsigned long long o = t >= d ? s_sum[t - d] : 0ull;
        __syncthreads();
        s_sum[t] += o;
        __syncthreads();
    }
    unsigned long long run = s_sum[t] - sum;
    for (int k = 0; k < per; ++k)
        if (a + k < n_tiles) {
            tile_start[a + k] = (unsigned)run;       // (a total that does not fit is refused by the host before these are used)
            cursor[a + k] = (unsigned)run;
            run += tile_count[a + k];
        }
    if (t == 1023) { counters[2] = (int)(unsigned)(s_sum[t] & 0xffffffffull); counters[3] = (int)(unsigned)(s_sum[t] >> 32); }
}

__global__ void __launch_bounds__(kWg) k_mr_bin(const View v, const long long n_lines, const int4* __restrict__ px, unsigned* __restrict__ cursor,
                                                unsigned* __restrict__ list)
{
    const long long i = (long long)blockIdx.x * kWg + threadIdx.x;
    const int lane = threadIdx.x & 63;
    int4 p = make_int4(kNotDrawn, 0, 0, 0);
    if (i < n_lines) p = px[i];
    TileIter it;
    bool more = p.x != kNotDrawn;
    if (more) it.init(p, v);
    unsigned tile = 0;
    for (;;) {
        if (more) more = it.next(tile);
        if (!__any(more)) break;
        const unsigned pos = wave_add(cursor, tile, more, lane);
        if (more) list[pos] = (unsigned)i;
    }
}

__global__ void __launch_bounds__(kWg) k_mr_paint(const View v, const int capacity, const uint8_t* __restrict__ color,
                                                  const int* __restrict__ last_seen, const int4* __restrict__ px,
                                                  const unsigned* __restrict__ tile_start, const unsigned* __restrict__ tile_count,
                                                  const unsigned* __restrict__ list, uint8_t* __restrict__ out)
{
    __shared__ unsigned long long plane[kTile * kTile];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int tx = blockIdx.x % v.ntx, ty = blockIdx.x / v.ntx;
    const int c0 = tx * kTile, r0 = ty * kTile;
    const int c1 = c0 + kTile - 1 < v.cols - 1 ? c0 + kTile - 1 : v.cols - 1, r1 = r0 + kTile - 1 < v.rows - 1 ? r0 + kTile - 1 : v.rows - 1;
    const int h0 = (v.thickness - 1) / 2, h1 = v.thickness / 2;
    for (int q = tid; q < kTile * kTile; q += kWg) plane[q] = 0ull;
    __syncthreads();
    const unsigned beg = tile_start[blockIdx.x], n_rec = tile_count[blockIdx.x];
    // 64 records a wave at a time; their (line, step) pairs are dealt to the lanes in order, so that a long line among short ones
    // keeps no lane waiting: pair `item` belongs to the first record whose inclusive step count exceeds it
    for (unsigned base = (unsigned)wave * 64u; base < n_rec; base += kWg) {
        int4 p = make_int4(0, 0, 0, 0);
        unsigned long long key = 0ull;
        int cnt = 0, i0 = 0;
        if (base + lane < n_rec) {
            const unsigned line = list[beg + base + lane];
            p = px[line];
            key = line < (unsigned)capacity ? entry_key(last_seen[line], line) : kTrajBit | (unsigned long long)(line - (unsigned)capacity + 1u);
            const Line L = make_line(p);
            long long ia, ib;
            if (step_range(L, (long long)(L.xmajor ? c0 : r0) - h1, (long long)(L.xmajor ? c1 : r1) + h0, ia, ib)) { cnt = (int)(ib - ia + 1); i0 = (int)ia; }
        }
        int inc = cnt;
        for (int d = 1; d < 64; d <<= 1) { const int o = __shfl_up(inc, d); if (lane >= d) inc += o; }
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
    __syncthreads();
    // the colours, in place: b | g << 8 | r << 16
    for (int q = tid; q < kTile * kTile; q += kWg) {
        const unsigned long long key = plane[q];
        unsigned bgr = v.bg;
        if (key & kTrajBit) bgr = 0x0000ffu;                                       // blue (odometry.py:59-61)
        else if (key) {
            const unsigned c = color[(unsigned)(key & 0x3fffffull) - 1u];          // show_map.py:59-70
            bgr = c == 0u ? 0xffffffu : c == 1u ? 0xffff00u : 0xff0000u;
        }
        plane[q] = bgr;
    }
    __syncthreads();
    // a tile row is up to 192 bytes of the image: a lane writes the aligned dword it lies in whole, or its bytes at the two ends
    const int nbytes = (c1 - c0 + 1) * 3;
    for (int r = wave; r0 + r <= r1; r += kWg / 64) {
        const uintptr_t a0 = reinterpret_cast<uintptr_t>(out) + ((size_t)(r0 + r) * v.cols + c0) * 3;
        const uintptr_t word = (a0 & ~(uintptr_t)3) + 4u * (unsigned)lane;
        unsigned val = 0, in = 0;
        for (int k = 0; k < 4; ++k) {
            const long long off = (long long)(word + k) - (long long)a0;
            if (off >= 0 && off < nbytes) {
                const int pix = (int)off / 3, ch = (int)off - 3 * pix;
                val |= (((unsigned)plane[r * kTile + pix] >> (8 * ch)) & 255u) << (8 * k);
                in |= 1u << k;
            }
        }
        if (in == 15u) *reinterpret_cast<unsigned*>(word) = val;
        else
            for (int k = 0; k < 4; ++k) if ((in >> k) & 1u) *reinterpret_cast<uint8_t*>(word + k) = (uint8_t)(val >> (8 * k));
    }
}

__global__ void __launch_bounds__(kWg) k_mr_bounds(const View v, const int has_view, const int capacity, const int* __restrict__ state,
                                                   const uint8_t* __restrict__ color, const double* __restrict__ ground,
                                                   const int* __restrict__ hits, const int* __restrict__ last_seen,
                                                   unsigned long long* __restrict__ res)
{
    const int i = blockIdx.x * kWg + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const double inf = __builtin_huge_val();
    double xmin = inf, ymin = inf, xmax = -inf, ymax = -inf;
    bool any = false;
    if (i < capacity && i < state[0] && (!has_view || selected(v, hits[i], last_seen[i], color[i])))
        for (int e = 0; e < 2; ++e) {
            const double x = ground[(size_t)i * 4 + 2 * e], y = ground[(size_t)i * 4 + 2 * e + 1];
            if (fabs(x) < inf && fabs(y) < inf) {
                any = true;
                xmin = fmin(xmin, x); xmax = fmax(xmax, x); ymin = fmin(ymin, y); ymax = fmax(ymax, y);
            }
        }
    const unsigned long long b = __ballot(any);
    if (!b) return;
    for (int d = 32; d; d >>= 1) {
        xmin = fmin(xmin, __shfl_xor(xmin, d)); ymin = fmin(ymin, __shfl_xor(ymin, d));
        xmax = fmax(xmax, __shfl_xor(xmax, d)); ymax = fmax(ymax, __shfl_xor(ymax, d));
    }
    if (lane == 0) {
        atomicMin(&res[0], encode_bound(xmin)); atomicMin(&res[1], encode_bound(ymin));
        atomicMax(&res[2], encode_bound(xmax)); atomicMax(&res[3], encode_bound(ymax));
        atomicAdd(&res[4], (unsigned long long)__popcll(b));
    }
}

}  // namespace

void launch_project(const View& v, const MapDevice& md, const double* traj, long long n_traj_lines, int4* px, unsigned* tile_count,
                    int* counters, hipStream_t s)
{
    const long long n = (long long)md.capacity + n_traj_lines;
    k_mr_project<<<dim3((unsigned)((n + kWg - 1) / kWg)), dim3(kWg), 0, s>>>(v, md.capacity, md.state, md.color, md.ground, md.hits, md.last_seen,
                                                                             traj, n_traj_lines, px, tile_count, counters);
}

void launch_scan(int n_tiles, const unsigned* tile_count, unsigned* tile_start, unsigned* cursor, int* counters, hipStream_t s)
{
    k_mr_scan<<<dim3(1), dim3(1024), 0, s>>>(n_tiles, tile_count, tile_start, cursor, counters);
}

void launch_bin(const View& v, const MapDevice& md, long long n_traj_lines, const int4* px, unsigned* cursor, unsigned* list, hipStream_t s)
{
    const long long n = (long long)md.capacity + n_traj_lines;
    k_mr_bin<<<dim3((unsigned)((n + kWg - 1) / kWg)), dim3(kWg), 0, s>>>(v, n, px, cursor, list);
}

void launch_paint(const View& v, const MapDevice& md, const int4* px, const unsigned* tile_start, const unsigned* tile_count,
                  const unsigned* list, uint8_t* out, hipStream_t s)
{
    k_mr_paint<<<dim3((unsigned)(v.ntx * v.nty)), dim3(kWg), 0, s>>>(v, md.capacity, md.color, md.last_seen, px, tile_start, tile_count, list, out);
}

void launch_bounds(const View& v, int has_view, const MapDevice& md, unsigned long long* res, hipStream_t s)
{
    k_mr_bounds<<<dim3((unsigned)((md.capacity + kWg - 1) / kWg)), dim3(kWg), 0, s>>>(v, has_view, md.capacity, md.state, md.color, md.ground,
                                                                                      md.hits, md.last_seen, res);
}

}  // namespace mr
}  // namespace lf
