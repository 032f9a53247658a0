// lf_map_align's kernel (include/lanefront.h "lf_map_align" is the contract; every f64 operation below is the header's, in its
// order, and this translation unit is built with -ffp-contract=off).
//
// One wave per frame, one launch for all frames and all iterations.  Lane l owns the contract's partial sum l: it walks the
// segments o0 + l, o0 + l + 64, ... in increasing order, endpoint 0 before endpoint 1, which is the stated order of summation.
// The pair data of a lane's FIRST segment (the segment's endpoints, the matched entry's normal and first endpoint, gathered
// through idx) stays in registers over the iterations: a frame of up to 64 segments reads memory once.  The segments beyond
// the first 64 of a longer frame are gathered again in every iteration (L2 hits: a frame's pairs are a few KB).  The fold is the
// contract's, through cross-lane moves; lane 0's sums are then broadcast and every lane solves the 3 x 3 system redundantly,
// so control flow stays uniform and no LDS is used.
#include "k_map_pairs.h"

namespace lf {
namespace ma {

__global__ __launch_bounds__(kPartials) void k_map_align(lf_align_config c, MapDevice md, Batch b)
{
    const int f = blockIdx.x, lane = threadIdx.x;
    if (f >= b.n_frames) return;
    const int size = map_size(md);
    const PairRule rule = { c.min_hits, c.color_match, c.max_dist };
    // frame_range's statements, spelled out: through the helper the register allocator ends two VGPRs above 128 and the kernel
    // one wave per SIMD lower
    int o0 = 0, o1 = 0;
    if (b.frame_offset && b.n > 0) {
        o0 = b.frame_offset[f]; o1 = b.frame_offset[f + 1];
        o0 = o0 < 0 ? 0 : (o0 > b.n ? b.n : o0);
        o1 = o1 < o0 ? o0 : (o1 > b.n ? b.n : o1);
    }
    const double x0 = b.pose0[3 * f], y0 = b.pose0[3 * f + 1], th0 = b.pose0[3 * f + 2];

    // the lane's first segment stays in registers; the pairs of the frame are counted once
    Pair first = no_pair();
    int mine = 0;
    if (o0 + lane < o1) { first = gather(rule, md, b, o0 + lane, size); mine = first.ok ? 1 : 0; }
    for (int i = o0 + lane + kPartials; i < o1; i += kPartials) mine += gather(rule, md, b, i, size).ok ? 1 : 0;
    const int n_pairs = fold(mine);

    double x = x0, y = y0, th = th0, cost0 = 0.0, cost = 0.0;
    int n_used = 0, accepted = 0, status = LF_ALIGN_OK;
    for (int k = 0; k < c.iterations; ++k) {
        double sn, cs;
        dm::dsincos(th, sn, cs);
        Sums s;
        clear(s);
        add_pair(s, c, first, x, y, sn, cs);
        for (int i = o0 + lane + kPartials; i < o1; i += kPartials) add_pair(s, c, gather(rule, md, b, i, size), x, y, sn, cs);
        fold(s);
        if (k == 0) cost0 = s.cost;
        cost = s.cost; n_used = s.used;
        if (s.used < 2 * c.min_pairs) { status = LF_ALIGN_FEW; break; }
        double t0, t1, t2;
        if (!solve(c, s, x, y, th, x0, y0, th0, t0, t1, t2)) { status = LF_ALIGN_DEGENERATE; break; }
        x += t0; y += t1; th += t2;
        accepted += 1;
    }
    const double ddx = x - x0, ddy = y - y0;
    const double shift = dm::dsqrt(ddx * ddx + ddy * ddy), turn = __builtin_fabs(th - th0);
    if (shift > c.max_shift || turn > c.max_turn) { status = LF_ALIGN_REJECTED; x = x0; y = y0; th = th0; }
    if (lane == 0) {
        double sn, cs;
        dm::dsincos(th, sn, cs);
        double* p4 = b.pose4 + 4 * (size_t)f;
        p4[0] = x; p4[1] = y; p4[2] = cs; p4[3] = sn;
        lf_align_result r;
        r.x = x; r.y = y; r.theta = th; r.cost0 = cost0; r.cost = cost;
        r.n_pairs = n_pairs; r.n_used = n_used; r.iterations = accepted; r.status = status;
        b.res[f] = r;
    }
}

void launch_align(const lf_align_config& c, const MapDevice& md, const Batch& b, hipStream_t s)
{
    hipLaunchKernelGGL(k_map_align, dim3(b.n_frames), dim3(kPartials), 0, s, c, md, b);
}

}  // namespace ma
}  // namespace lf
