// Host side of GroundProjection.rectify (k_rectify.hip) and of the camera a live handle projects with: the undistortion map in
// strict float64 (this file is built with -ffp-contract=off like every other), its fixed-point form and the bicubic weight table on
// the device, the launches; lf_set_camera and lf_set_rectified_input.  Every statement of the map and the table has its twin in
// tests/rectify_ref.py, which says what it was restated from.
#include <math.h>
#include <string.h>
#include <limits.h>
#include <stdlib.h>
#include <vector>
#include "lanefront_handle.h"
#include "k_rectify.h"

using namespace lf;

namespace {

constexpr int kMaxSide = 8192;
constexpr int kMaxFrames = 65535;     // a grid dimension
constexpr long kSplitTarget = 8192;   // workgroups a launch aims for (lf_rectify_batch; measured)

// cv::invert(DECOMP_LU) of a 3 x 3 double matrix: the closed form.  false: the determinant is 0 (or not a number)
bool invert3(const double* m, double* t)
{
    double d = m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
    if (!(d != 0.) || !isfinite(d)) return false;
    d = 1. / d;
    t[0] = (m[4] * m[8] - m[5] * m[7]) * d;
    t[1] = (m[2] * m[7] - m[1] * m[8]) * d;
    t[2] = (m[1] * m[5] - m[2] * m[4]) * d;
    t[3] = (m[5] * m[6] - m[3] * m[8]) * d;
    t[4] = (m[0] * m[8] - m[2] * m[6]) * d;
    t[5] = (m[2] * m[3] - m[0] * m[5]) * d;
    t[6] = (m[3] * m[7] - m[4] * m[6]) * d;
    t[7] = (m[1] * m[6] - m[0] * m[7]) * d;
    t[8] = (m[0] * m[4] - m[1] * m[3]) * d;
    return true;
}

void projection_rotation(const double* R, const double* P, double* out)
{
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) out[3 * i + j] = P[4 * i] * R[j] + P[4 * i + 1] * R[3 + j] + P[4 * i + 2] * R[6 + j];
}

// initUndistortRectifyMap(K, D, R, P, (w, h), CV_32FC1): sink(i, j, mapx, mapy) for every pixel, rows in order
template <typename Sink>
bool for_each_map_pixel(const lf_config& c, Sink sink)
{
    double PR[9], iR[9];
    projection_rotation(c.R, c.P, PR);
    if (!invert3(PR, iR)) return false;
    const double fx = c.K[0], fy = c.K[4], u0 = c.K[2], v0 = c.K[5];
    const double k1 = c.D[0], k2 = c.D[1], p1 = c.D[2], p2 = c.D[3], k3 = c.D[4];
    for (int i = 0; i < c.cam_h; ++i) {
        double _x = i * iR[1] + iR[2], _y = i * iR[4] + iR[5], _w = i * iR[7] + iR[8];
        for (int j = 0; j < c.cam_w; ++j, _x += iR[0], _y += iR[3], _w += iR[6]) {
            const double w = 1. / _w, x = _x * w, y = _y * w;
            const double x2 = x * x, y2 = y * y;
            const double r2 = x2 + y2, _2xy = 2 * x * y;
            const double kr = 1 + ((k3 * r2 + k2) * r2 + k1) * r2;
            const double u = fx * (x * kr + p1 * _2xy + p2 * (r2 + 2 * x2)) + u0;
            const double v = fy * (y * kr + p1 * (r2 + 2 * y2) + p2 * _2xy) + v0;
            sink(i, j, (float)u, (float)v);
        }
    }
    return true;
}

// cvRound(m * INTER_TAB_SIZE), the product in float32: cvtss2si's INT_MIN for a NaN and for a value outside int32
int cv_round_x32(float m)
{
    const float v = m * (float)rect::kInterTab;
    if (!(v >= -2147483648.f && v < 2147483648.f)) return INT_MIN;
    return (int)nearbyint((double)v);              // round half to even
}
int saturate_short(int v) { return v < -32768 ? -32768 : v > 32767 ? 32767 : v; }

// interpolateCubic(x, coeffs), A = -0.75, in float32
void interpolate_cubic(float x, float* c)
{
    const float A = -0.75f;
    c[0] = ((A * (x + 1) - 5 * A) * (x + 1) + 8 * A) * (x + 1) - 4 * A;
    c[1] = ((A + 2) * x - (A + 3)) * x * x + 1;
    c[2] = ((A + 2) * (1 - x) - (A + 3)) * (1 - x) * (1 - x) + 1;
    c[3] = 1.f - c[0] - c[1] - c[2];
}

// initInterTab2D(INTER_CUBIC, fixpt): [kTabRows][4][4] int16; the sum correction is tests/rectify_ref.py's _fix_sum
void make_table(int16_t* tab)
{
    float one_d[rect::kInterTab][4];
    for (int i = 0; i < rect::kInterTab; ++i) interpolate_cubic((float)i * (1.f / rect::kInterTab), one_d[i]);
    for (int i = 0; i < rect::kInterTab; ++i)
        for (int j = 0; j < rect::kInterTab; ++j) {
            int it[4][4], sum = 0;
            for (int k1 = 0; k1 < 4; ++k1)
                for (int k2 = 0; k2 < 4; ++k2) {
                    const float v = one_d[i][k1] * one_d[j][k2];
                    sum += it[k1][k2] = saturate_short((int)nearbyint((double)(v * (float)(1 << rect::kCoefBits))));
                }
            const int diff = sum - (1 << rect::kCoefBits);
            if (diff) {
                int Mk1 = 1, Mk2 = 1, mk1 = 1, mk2 = 1;
                for (int k1 = 1; k1 < 3; ++k1)
                    for (int k2 = 1; k2 < 3; ++k2) {
                        if (it[k1][k2] < it[mk1][mk2]) { mk1 = k1; mk2 = k2; }
                        else if (it[k1][k2] > it[Mk1][Mk2]) { Mk1 = k1; Mk2 = k2; }
                    }
                if (diff > 0) it[Mk1][Mk2] -= diff; else it[mk1][mk2] -= diff;
            }
            int16_t* o = tab + ((size_t)i * rect::kInterTab + j) * 16;
            for (int k = 0; k < 16; ++k) o[k] = (int16_t)it[k >> 2][k & 3];
        }
}

bool camera_ok(lf_handle* h, const char* who, const lf_config& c)
{
    if (c.cam_w < 1 || c.cam_h < 1 || c.cam_w > kMaxSide || c.cam_h > kMaxSide) {
        lf_set_error(h, LF_ERR_BAD_ARG, "%s: a camera of %d x %d (1 .. %d px a side)", who, c.cam_w, c.cam_h, kMaxSide);
        return false;
    }
    double PR[9], iR[9];
    projection_rotation(c.R, c.P, PR);
    if (!invert3(PR, iR)) { lf_set_error(h, LF_ERR_BAD_ARG, "%s: P[:3,:3] . R is singular", who); return false; }
    return true;
}

// the handle's map and table on the device, made for its camera as it is now
int ensure_map(lf_handle* h, const char* who)
{
    if (!h->rect) h->rect.reset(new RectState());
    RectState& e = *h->rect;
    if (e.map_ready) return LF_OK;
    const lf_config& c = h->cfg;
    if (!camera_ok(h, who, c)) return LF_ERR_BAD_ARG;
    const size_t px = (size_t)c.cam_w * c.cam_h;
    // (kernels of an earlier call may still read the map that is about to be replaced)
    LF_HIP_CHECK(h, hipStreamSynchronize(h->stream));
    int rc;
    if ((rc = scratch(h, e.xy, px * sizeof(short2))) || (rc = scratch(h, e.frac, px * sizeof(uint16_t)))) return rc;
    if (!e.tab.p) {
        std::vector<int16_t> tab((size_t)rect::kTabRows * 16);
        make_table(tab.data());
        LF_HIP_CHECK(h, e.tab.alloc(tab.size() * sizeof(int16_t)));
        LF_HIP_CHECK(h, hipMemcpy(e.tab.p, tab.data(), tab.size() * sizeof(int16_t), hipMemcpyHostToDevice));
    }
    std::vector<short2> xy(px);
    std::vector<uint16_t> frac(px);
    const int w = c.cam_w;
    for_each_map_pixel(c, [&](int i, int j, float mx, float my) {
        const int sx = cv_round_x32(mx), sy = cv_round_x32(my);
        const size_t p = (size_t)i * w + j;
        xy[p].x = (short)saturate_short(sx >> rect::kInterBits);
        xy[p].y = (short)saturate_short(sy >> rect::kInterBits);
        frac[p] = (uint16_t)((sy & (rect::kInterTab - 1)) * rect::kInterTab + (sx & (rect::kInterTab - 1)));
    });
    LF_HIP_CHECK(h, hipMemcpy(e.xy.p, xy.data(), px * sizeof(short2), hipMemcpyHostToDevice));
    LF_HIP_CHECK(h, hipMemcpy(e.frac.p, frac.data(), px * sizeof(uint16_t), hipMemcpyHostToDevice));
    e.w = c.cam_w; e.h = c.cam_h;
    e.map_ready = true;
    e.maps_built += 1;
    return LF_OK;
}

bool overlap(const void* a, size_t na, const void* b, size_t nb)
{
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a0 < b0 + nb && b0 < a0 + na;
}

}  // namespace

// ---- the camera of a live handle (GroundProjection.initialize_pinhole_camera_model, GroundProjection.py:33-36)
extern "C" int lf_set_camera(lf_handle* h, const double* K, const double* D, const double* R, const double* P, int cam_w, int cam_h)
{
    if (!h) return LF_ERR_NOT_INITIALISED;
    if (!K || !D || !R || !P) { lf_set_error(h, LF_ERR_BAD_ARG, "lf_set_camera: null argument"); return LF_ERR_BAD_ARG; }
    if (const int rc = refuse_in_flight(h)) return rc;
    lf_config c = h->cfg;
    memcpy(c.K, K, sizeof(c.K)); memcpy(c.D, D, sizeof(c.D)); memcpy(c.R, R, sizeof(c.R)); memcpy(c.P, P, sizeof(c.P));
    c.cam_w = cam_w; c.cam_h = cam_h;
    if (!camera_ok(h, "lf_set_camera", c)) return LF_ERR_BAD_ARG;
    h->cfg = c;
    seg_camera(h);
    if (h->rect) h->rect->map_ready = false;
    return LF_OK;
}

// ---- GroundProjection.rectified_input (GroundProjection.py:21,66-67)
extern "C" int lf_set_rectified_input(lf_handle* h, int flag)
{
    if (!h) return LF_ERR_NOT_INITIALISED;
    if (const int rc = refuse_in_flight(h)) return rc;
    h->seg.rectified_input = flag ? 1 : 0;
    return LF_OK;
}

extern "C" int lf_get_rectified_input(lf_handle* h, int* flag)
{
    if (!h) return LF_ERR_NOT_INITIALISED;
    if (!flag) { lf_set_error(h, LF_ERR_BAD_ARG, "lf_get_rectified_input: null argument"); return LF_ERR_BAD_ARG; }
    *flag = h->seg.rectified_input;
    return LF_OK;
}

extern "C" int lf_rectify_map(lf_handle* h, float* mapx, float* mapy)
{
    if (!h) return LF_ERR_NOT_INITIALISED;
    if (!mapx || !mapy) { lf_set_error(h, LF_ERR_BAD_ARG, "lf_rectify_map: null argument"); return LF_ERR_BAD_ARG; }
    const lf_config& c = h->cfg;
    if (!camera_ok(h, "lf_rectify_map", c)) return LF_ERR_BAD_ARG;
    const int w = c.cam_w;
    for_each_map_pixel(c, [&](int i, int j, float mx, float my) { mapx[(size_t)i * w + j] = mx; mapy[(size_t)i * w + j] = my; });
    return LF_OK;
}

extern "C" int lf_rectify_batch(lf_handle* h, const uint8_t* src, int src_on_device, int n_frames, int rows, int cols, int channels, uint8_t* dst,
                                int dst_on_device)
{
    if (!h) return LF_ERR_NOT_INITIALISED;
    if (!src || !dst) { lf_set_error(h, LF_ERR_BAD_ARG, "lf_rectify_batch: null argument"); return LF_ERR_BAD_ARG; }
    if (n_frames < 1 || n_frames > kMaxFrames) {
        lf_set_error(h, LF_ERR_BAD_ARG, "lf_rectify_batch: n_frames %d (1 .. %d)", n_frames, kMaxFrames);
        return LF_ERR_BAD_ARG;
    }
    if (rows < 1 || cols < 1 || rows > kMaxSide || cols > kMaxSide) {
        lf_set_error(h, LF_ERR_BAD_ARG, "lf_rectify_batch: frames of %d x %d (1 .. %d px a side)", rows, cols, kMaxSide);
        return LF_ERR_BAD_ARG;
    }
    if (channels != 1 && channels != 3) { lf_set_error(h, LF_ERR_BAD_ARG, "lf_rectify_batch: %d channels (1 or 3)", channels); return LF_ERR_BAD_ARG; }
    const lf_config& c = h->cfg;
    if (!camera_ok(h, "lf_rectify_batch", c)) return LF_ERR_BAD_ARG;
    const size_t n = (size_t)n_frames;
    const size_t src_bytes = n * rows * cols * channels, dst_bytes = n * c.cam_h * c.cam_w * channels;
    if (!src_on_device == !dst_on_device && overlap(src, src_bytes, dst, dst_bytes)) {
        lf_set_error(h, LF_ERR_BAD_ARG, "lf_rectify_batch: dst overlaps src (remap does not work in place)");
        return LF_ERR_BAD_ARG;
    }
    LF_HIP_CHECK(h, hipSetDevice(h->device));
    int rc;
    if ((rc = ensure_map(h, "lf_rectify_batch")) != LF_OK) return rc;
    RectState& e = *h->rect;
    hipStream_t s = h->stream;
    Staging st(h);
    const uint8_t* d_src = st.in(src_on_device, src, src_bytes, e.in);
    uint8_t* d_dst = st.out(dst_on_device, dst, dst_bytes, e.out);
    if ((rc = st.upload()) != LF_OK) return rc;
    rect::Map m;
    m.xy = static_cast<const short2*>(e.xy.p); m.frac = static_cast<const uint16_t*>(e.frac.p); m.tab = static_cast<const int16_t*>(e.tab.p);
    m.w = e.w; m.h = e.h;
    // Workgroups that share a tile's frames: a tile per workgroup alone is 300 workgroups for a 640 x 480 camera, a wave or so per
    // SIMD on a chip whose gather wants every wave slot busy; the map is read once per workgroup, so the split costs 6 bytes per
    // pixel each.  LF_RECTIFY_SPLIT=<workgroups per tile> overrides (tools/rectify_rate.py).
    const long tiles = (long)((m.w + rect::kTileW - 1) / rect::kTileW) * ((m.h + rect::kTileH - 1) / rect::kTileH);
    long split = (kSplitTarget + tiles - 1) / tiles;
    const char* env_split = getenv("LF_RECTIFY_SPLIT");     // (read per call: the tool sweeps it in one process)
    if (env_split && atol(env_split) > 0) split = atol(env_split);
    if (split > n_frames) split = n_frames;
    if (split > (1L << 30) / tiles) split = (1L << 30) / tiles;
    if (split < 1) split = 1;
    if ((rc = e.clock.begin(h)) != LF_OK) return rc;
    {
        CallClock::Scope t(e.clock, 0);
        rect::launch_remap(m, d_src, n_frames, rows, cols, channels, d_dst, (int)split, s);
    }
    LF_HIP_CHECK(h, hipGetLastError());
    return fetch(h, { { dst, d_dst, dst_bytes } });
}

extern "C" int lf_rectify_timing(lf_handle* h, double* ms_per_stage, int n)
{
    if (!h) return LF_ERR_NOT_INITIALISED;
    if (!ms_per_stage || n < rect::kStages) { lf_set_error(h, LF_ERR_BAD_ARG, "lf_rectify_timing: room for %d stages", rect::kStages); return LF_ERR_BAD_ARG; }
    if (!h->rect || !h->rect->clock.timed) {
        lf_set_error(h, LF_ERR_BAD_ARG, "lf_rectify_timing: no lf_rectify_batch ran with profiling on (lf_set_profiling)");
        return LF_ERR_BAD_ARG;
    }
    return h->rect->clock.read(h, rect::kStages, ms_per_stage);
}

extern "C" const char* lf_rectify_stage_name(int stage)
{
    return stage == 0 ? "k_rectify" : "";
}
