// lf_map_render_camera: the live map (k_map.hip) drawn into rectified camera frames, what the reference's augmented reality
// (duckietown_utils/augmented_reality_utils.py, BaseAugmenter.render_segments) draws with cv2.line at the pixels of
// GroundProjection.ground2pixel's rectified branch (GroundProjection.py:80-93): Hinv . (x, y, 1), normalised.  The reference leaves
// both ground2pixel bodies empty, so the pixel contract is the package's own (include/lanefront.h "lf_map_render_camera";
// tests/map_camera_ref.py restates it sequentially):
//   robot frame        dx = X - x, dy = Y - y, px = cs dx + sn dy, py = cs dy - sn dx      (f64, unfused: built -ffp-contract=off)
//   homogeneous pixel  q_k = (h_k0 px + h_k1 py) + h_k2
//   near plane         q_z < w_near at both ends: behind; at one end: that end moves along the segment to q_z = w_near
//   pixel              u = floor((q_x / q_z) sx), v = floor((q_y / q_z) sy) - top_cutoff
//   line, brush, winner  k_map_raster.h, as lf_map_render
// A batch of frames shares the map and differs in the pose, so the tile lists are per (frame, tile).  Nothing the size of frames x
// capacity is kept: 1 project counts the tiles of every (frame, entry), 2 the scan of k_map_render.hip, 3 project again, now writing
// each (line, tile) pair with its pixel endpoints, 4 paint, one workgroup per (frame, tile): the winners on an LDS plane, then the
// source tile with the painted pixels replaced.
#include "k_map_camera.h"
#include "k_map_raster.h"

namespace lf {
namespace mc {

namespace {

using mr::kTile;
using mr::kWg;

enum { kNone = 0, kDrawn = 1, kSkipped = 2, kBehind = 3 };

// the category of the entry with endpoints g at the pose (x, y, cs, sn), and the pixel endpoints of a drawn one
__device__ inline int project_entry(const View& v, const double* g, double x, double y, double cs, double sn, int4& p)
{
    double q[2][3];
    for (int e = 0; e < 2; ++e) {
        const double dx = g[2 * e] - x, dy = g[2 * e + 1] - y;
        const double px = cs * dx + sn * dy, py = cs * dy - sn * dx;
        for (int k = 0; k < 3; ++k) q[e][k] = (v.h[3 * k] * px + v.h[3 * k + 1] * py) + v.h[3 * k + 2];
    }
    const bool below_a = q[0][2] < v.w_near, below_b = q[1][2] < v.w_near;
    if (below_a && below_b) return kBehind;
    if (below_a || below_b) {
        const int e = below_a ? 0 : 1, o = 1 - e;
        const double t = (v.w_near - q[e][2]) / (q[o][2] - q[e][2]);
        q[e][0] = q[e][0] + t * (q[o][0] - q[e][0]);
        q[e][1] = q[e][1] + t * (q[o][1] - q[e][1]);
        q[e][2] = v.w_near;
    }
    const double f[4] = { floor((q[0][0] / q[0][2]) * v.sx), floor((q[0][1] / q[0][2]) * v.sy),
                          floor((q[1][0] / q[1][2]) * v.sx), floor((q[1][1] / q[1][2]) * v.sy) };
    if (!(fabs(f[0]) < mr::kPixLimit && fabs(f[1]) < mr::kPixLimit && fabs(f[2]) < mr::kPixLimit && fabs(f[3]) < mr::kPixLimit)) return kSkipped;   // (a NaN too)
    p = make_int4((int)f[0], (int)f[1] - v.top_cutoff, (int)f[2], (int)f[3] - v.top_cutoff);
    return kDrawn;
}

// blockIdx.y = the frame, so a wave never spans two
template <bool kBin>
__global__ void __launch_bounds__(kWg) k_mc_project(const View v, const int capacity, const int* __restrict__ state,
                                                    const uint8_t* __restrict__ color, const double* __restrict__ ground,
                                                    const int* __restrict__ hits, const int* __restrict__ last_seen,
                                                    const double* __restrict__ pose4, unsigned* __restrict__ tile_ctr,
                                                    int* __restrict__ counters, Record* __restrict__ rec)
{
    const int i = blockIdx.x * kWg + threadIdx.x, f = blockIdx.y;
    const int lane = threadIdx.x & 63;
    int cat = kNone;
    int4 p = make_int4(0, 0, 0, 0);
    if (i < capacity && i < state[0] && mr::selected(v.min_hits, v.min_last_seen, v.color_mask, hits[i], last_seen[i], color[i])) {
        double g[4];
        for (int k = 0; k < 4; ++k) g[k] = ground[(size_t)i * 4 + k];
        cat = project_entry(v, g, pose4[4 * f], pose4[4 * f + 1], pose4[4 * f + 2], pose4[4 * f + 3], p);
    }
    if (!kBin) {
        const unsigned long long bd = __ballot(cat == kDrawn), bs = __ballot(cat == kSkipped), bb = __ballot(cat == kBehind);
        if (lane == 0) {
            int* c = counters + kCounterBase + 3 * f;
            if (bd) atomicAdd(&c[0], (int)__popcll(bd));
            if (bs) atomicAdd(&c[1], (int)__popcll(bs));
            if (bb) atomicAdd(&c[2], (int)__popcll(bb));
        }
    }
    unsigned* ctr = tile_ctr + (size_t)f * (unsigned)(v.ntx * v.nty);
    mr::TileIter it;
    bool more = cat == kDrawn;
    if (more) it.init(p, v.thickness, v.rows, v.cols, v.ntx);
    unsigned tile = 0;
    for (;;) {
        if (more) more = it.next(tile);
        if (!__any(more)) break;
        const unsigned pos = mr::wave_add(ctr, tile, more, lane);
        if (kBin && more) {
            Record r;
            r.px[0] = p.x; r.px[1] = p.y; r.px[2] = p.z; r.px[3] = p.w; r.slot = (unsigned)i;
            rec[pos] = r;
        }
    }
}

__global__ void __launch_bounds__(kWg) k_mc_paint(const View v, const uint8_t* __restrict__ color, const int* __restrict__ last_seen,
                                                  const unsigned* __restrict__ tile_start, const unsigned* __restrict__ tile_count,
                                                  const Record* __restrict__ rec, const uint8_t* src, uint8_t* out)
{
    __shared__ unsigned long long plane[kTile * kTile];
    const int tid = threadIdx.x;
    const int tx = blockIdx.x % v.ntx, ty = blockIdx.x / v.ntx;
    const size_t f = blockIdx.y, ft = f * (unsigned)(v.ntx * v.nty) + blockIdx.x;
    const unsigned beg = tile_start[ft], n_rec = tile_count[ft];
    if (!n_rec && src == out) return;                             // in place and nothing to paint: the tile is as it should be
    const int c0 = tx * kTile, r0 = ty * kTile;
    const int c1 = c0 + kTile - 1 < v.cols - 1 ? c0 + kTile - 1 : v.cols - 1, r1 = r0 + kTile - 1 < v.rows - 1 ? r0 + kTile - 1 : v.rows - 1;
    const int h0 = (v.thickness - 1) / 2, h1 = v.thickness / 2;
    for (int q = tid; q < kTile * kTile; q += kWg) plane[q] = 0ull;
    __syncthreads();
    mr::paint_records(plane, n_rec, c0, c1, r0, r1, h0, h1, [&](unsigned k, int4& p, unsigned long long& key) {
        const Record r = rec[beg + k];
        p = make_int4(r.px[0], r.px[1], r.px[2], r.px[3]);
        key = mr::entry_key(last_seen[r.slot], r.slot);
    });
    __syncthreads();
    // the colours, in place: b | g << 8 | r << 16, bit 24 = painted
    for (int q = tid; q < kTile * kTile; q += kWg) {
        const unsigned long long key = plane[q];
        unsigned bgr = v.bg;
        if (key) {
            const unsigned c = color[(unsigned)(key & 0x3fffffull) - 1u];
            bgr = v.palette[c < 7u ? c : 7u] | 1u << 24;
        }
        plane[q] = bgr;
    }
    __syncthreads();
    // The frame is the caller's: store_tile_rows writes no byte outside the tile's own, so the workgroups of neighbouring tiles never
    // meet in a dword.  Unpainted bytes come from src, whose alignment need not be out's; in place they are there already.
    const size_t frame_bytes = (size_t)v.rows * v.cols * 3;
    const bool in_place = src == out;
    const uint8_t* s0 = src ? src + f * frame_bytes + ((size_t)r0 * v.cols + c0) * 3 : nullptr;      // the tile's first byte
    mr::store_tile_rows(out + f * frame_bytes, v.cols, c0, c1, r0, r1, [&](int r, int pix, int ch, int off, unsigned& b) {
        const unsigned c = (unsigned)plane[r * kTile + pix];
        b = c >> (8 * ch);
        if (c >> 24) return true;
        if (in_place) return false;
        if (s0) b = s0[(size_t)r * v.cols * 3 + off];
        return true;
    });
}

}  // namespace

void launch_project(const View& v, const MapDevice& md, const double* pose4, int n_frames, unsigned* tile_count_or_cursor, int* counters,
                    Record* rec, hipStream_t s)
{
    const dim3 grid((unsigned)((md.capacity + kWg - 1) / kWg), (unsigned)n_frames);
    if (rec) k_mc_project<true><<<grid, dim3(kWg), 0, s>>>(v, md.capacity, md.state, md.color, md.ground, md.hits, md.last_seen, pose4,
                                                          tile_count_or_cursor, counters, rec);
    else k_mc_project<false><<<grid, dim3(kWg), 0, s>>>(v, md.capacity, md.state, md.color, md.ground, md.hits, md.last_seen, pose4,
                                                       tile_count_or_cursor, counters, rec);
}

void launch_paint(const View& v, const MapDevice& md, int n_frames, const unsigned* tile_start, const unsigned* tile_count, const Record* rec,
                  const uint8_t* src, uint8_t* out, hipStream_t s)
{
    k_mc_paint<<<dim3((unsigned)(v.ntx * v.nty), (unsigned)n_frames), dim3(kWg), 0, s>>>(v, md.color, md.last_seen, tile_start, tile_count, rec,
                                                                                       src, out);
}

}  // namespace mc
}  // namespace lf
