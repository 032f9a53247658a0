// Where the robot is in its lane, from the live map's polylines (include/lanefront.h "lf_map_lane_pose"; tests/map_lane_pose_ref.py
// is the sequential restatement; every f64 operation below is the header's, in its order, and this translation unit is built with
// -ffp-contract=off).  Behind pl::launch_polylines (k_map_polylines.hip), on the same stream.
//
//   k_lp_edges   one thread per vertex index: B, the edge it starts as a 44-byte record in six arrays (k_map_lane_pose.h Edges), and
//                n_edges[c] with one atomic per wave and colour (a ballot and its popcount)
//   k_lp_query   one workgroup of 256 per frame: the lanes stride over the edge records and each keeps its best (d2, i) per colour --
//                d2 as its bit pattern, which orders as an integer because a candidate's d2 is finite and not negative; the minimum
//                of the bits and then the minimum i among the lanes that hold it go down the wave's butterfly, the four waves meet in
//                LDS, and lane 0 works out D and E for the two winners again and writes the 96 bytes field by field
// Every loop runs to the number of vertices, read from the device counter and cut to the tables' length; nothing spins.
#include "k_map_lane_pose.h"
#include "detmath.h"
#include "wave.h"

namespace lf {
namespace lp {

namespace {

constexpr int kNone = 0x7fffffff;
constexpr long long kNoBits = 0x7fffffffffffffffll;      // above every finite double's bits (a NaN's: never a candidate's)

__device__ __forceinline__ int n_vertices(const Tables& t)
{
    const int nv = t.pl_counters[pl::kNVertices];
    return nv < t.bound ? nv : t.bound;
}

// C for edge i and one pose; everything D needs comes back
struct Hit { double d2, s, o, hd, hc, L2; };

__device__ __forceinline__ bool candidate(const Rule& c, const Edges& e, int i, int colour, double x, double y, double cs, double sn, Hit& h)
{
    const double ax = e.ax[i], ay = e.ay[i], bx = e.bx[i], by = e.by[i], L2 = e.L2[i];
    const double ux = bx - ax, uy = by - ay;
    const double px = x - ax, py = y - ay;
    const double t = px * ux + py * uy;
    double qx, qy;
    if (t <= 0.0) { qx = px; qy = py; }
    else if (t >= L2) { qx = x - bx; qy = y - by; }
    else {
        const double r = t / L2;
        qx = px - r * ux; qy = py - r * uy;
    }
    h.d2 = qx * qx + qy * qy;
    if (!(h.d2 <= c.r2)) return false;
    h.hd = cs * ux + sn * uy; h.hc = cs * uy - sn * ux;
    if (c.test_sin && !(h.hc * h.hc <= c.ms2 * L2)) return false;
    h.o = h.hd < 0.0 ? -1.0 : 1.0;
    h.s = (h.o * ux) * qy - (h.o * uy) * qx;
    h.L2 = L2;
    if (c.sides) return colour == 0 ? h.s > 0.0 : h.s < 0.0;
    return true;
}

}  // namespace

__global__ __launch_bounds__(kWg) void k_lp_edges(Rule c, MapDevice md, Tables t, Edges e)
{
    const int i = blockIdx.x * kWg + threadIdx.x;
    const int nv = n_vertices(t);
    int colour = -1;
    if (i < nv) {
        const lf_polyline_vertex* v = t.vertices + i;
        const int k = v->polyline, row = v->first_row;
        if (k >= 0 && k < t.bound && row >= 0 && row < md.capacity) {
            const lf_polyline* p = t.polylines + k;
            const int first = p->first_vertex, n = p->n_vertices;
            int j = -1;
            if (i + 1 < first + n) j = i + 1;
            else if (p->closed && n >= 3) j = first;
            if (j >= 0 && j < nv) {
                const double ax = v->x, ay = v->y, bx = t.vertices[j].x, by = t.vertices[j].y;
                const double ux = bx - ax, uy = by - ay;
                const double L2 = ux * ux + uy * uy;
                const int col = md.color[row];
                e.ax[i] = ax; e.ay[i] = ay; e.bx[i] = bx; e.by[i] = by; e.L2[i] = L2;
                if (col <= 1 && n >= c.min_vertices && L2 > 0.0) colour = col;
            }
        }
        e.colour[i] = colour;
    }
    // (no return above: the ballots see every lane of the wave)
#pragma unroll
    for (int col = 0; col < 2; ++col) {
        const int n = __popcll(wave_ballot(colour == col));
        if ((threadIdx.x & 63) == 0 && n) atomicAdd(t.counters + (col == 0 ? kNEdgesWhite : kNEdgesYellow), n);
    }
}

__global__ __launch_bounds__(kWg) void k_lp_query(Rule c, Tables t, Edges e, const double* pose4, lf_map_lane_pose_record* out)
{
    __shared__ long long s_bits[2][kWg / 64];
    __shared__ int s_at[2][kWg / 64];
    const int f = blockIdx.x;
    const int nv = n_vertices(t);
    const double x = pose4[4 * f], y = pose4[4 * f + 1], cs = pose4[4 * f + 2], sn = pose4[4 * f + 3];
    long long best[2] = { kNoBits, kNoBits };
    int at[2] = { kNone, kNone };
    for (int i = threadIdx.x; i < nv; i += kWg) {
        const int colour = e.colour[i];
        if (colour < 0) continue;
        Hit h;
        if (!candidate(c, e, i, colour, x, y, cs, sn, h)) continue;
        const long long bits = __double_as_longlong(h.d2);
        // (i grows in a lane: on equal bits the earlier edge stays)
        if (colour == 0) { if (bits < best[0]) { best[0] = bits; at[0] = i; } }
        else if (bits < best[1]) { best[1] = bits; at[1] = i; }
    }
    // all 256 lanes are here again, the ones without a candidate with the neutral elements
#pragma unroll
    for (int col = 0; col < 2; ++col) {
        const long long m = wave_reduce<64>(best[col], op_min());
        const int a = wave_reduce<64>(best[col] == m ? at[col] : kNone, op_min());
        if ((threadIdx.x & 63) == 0) { s_bits[col][threadIdx.x >> 6] = m; s_at[col][threadIdx.x >> 6] = a; }
    }
    __syncthreads();
    if (threadIdx.x != 0) return;

    lf_map_lane_pose_record* r = out + f;
    double l[2] = { 0.0, 0.0 }, ld[2] = { 0.0, 0.0 }, lphi[2] = { 0.0, 0.0 };
    int status = 0;
#pragma unroll
    for (int col = 0; col < 2; ++col) {
        long long m = kNoBits;
        int i = kNone;
        for (int wv = 0; wv < kWg / 64; ++wv)
            if (s_bits[col][wv] < m || (s_bits[col][wv] == m && s_at[col][wv] < i)) { m = s_bits[col][wv]; i = s_at[col][wv]; }
        Hit h;
        double line_dist = 0.0;
        int vertex = -1, polyline = -1;
        if (i != kNone && i >= 0 && i < nv && candidate(c, e, i, col, x, y, cs, sn, h)) {
            line_dist = dm::dsqrt(h.d2);
            l[col] = h.s / dm::dsqrt(h.L2);
            ld[col] = l[col] + c.offset[col];
            lphi[col] = dm::datan2(-(h.o * h.hc), h.o * h.hd);
            vertex = i; polyline = t.vertices[i].polyline;
            status |= 1 << col;
        }
        r->line_d[col] = ld[col] + 0.0; r->line_phi[col] = lphi[col] + 0.0; r->line_dist[col] = line_dist + 0.0;
        r->vertex[col] = vertex; r->polyline[col] = polyline;
    }
    double d = 0.0, phi = 0.0, width = 0.0;
    if (status == 3) {
        d = (ld[0] + ld[1]) * 0.5; phi = (lphi[0] + lphi[1]) * 0.5;
        width = l[0] - l[1];
    } else if (status != 0) {
        d = ld[status >> 1]; phi = lphi[status >> 1];
    }
    r->d = d + 0.0; r->phi = phi + 0.0; r->width = width + 0.0;
    r->status = status;
    r->in_lane = status != 0 && __builtin_fabs(d) <= c.max_d ? 1 : 0;
    if (status != 0) atomicAdd(t.counters + kNPosed, 1);
}

void launch_edges(const Rule& c, const MapDevice& md, const Tables& t, const Edges& e, hipStream_t s)
{
    hipLaunchKernelGGL(k_lp_edges, dim3((t.bound + kWg - 1) / kWg), dim3(kWg), 0, s, c, md, t, e);
}

void launch_query(const Rule& c, const Tables& t, const Edges& e, const double* pose4, int n_frames, lf_map_lane_pose_record* out, hipStream_t s)
{
    hipLaunchKernelGGL(k_lp_query, dim3(n_frames), dim3(kWg), 0, s, c, t, e, pose4, out);
}

}  // namespace lp
}  // namespace lf
