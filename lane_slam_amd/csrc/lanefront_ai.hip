// Host side of the anti-instagram estimate (k_ai.hip), the setter of the transform k_pre applies, and the colour clustering the
// estimate is made of as an entry point of its own (lf_kmeans, k_kmeans.hip).
#include <math.h>
#include "lanefront_handle.h"

using namespace lf;

extern "C" int lf_ai_transform_batch(lf_handle* h, const uint8_t* frames, int n_frames, int frames_on_device, int rows, int cols,
                                     lf_ai_transform* out)
{
    if (!h) return LF_ERR_NOT_INITIALISED;
    if (!frames || !out || n_frames < 1 || rows < 1 || cols < 1) {
        lf_set_error(h, LF_ERR_BAD_ARG, "lf_ai_transform_batch: null argument, n_frames < 1 or an empty frame (%d x %d)", rows, cols);
        return LF_ERR_BAD_ARG;
    }
    if (const int rc = refuse_in_flight(h)) return rc;
    const int S = rows < 100 ? rows : 100;                     // image[-100:] (kmeans.py:24)
    const long long n = (long long)S * cols;
    if (n > (1 << 24)) {      // the limit of lf_kmeans (k_kmeans.h: per-wave 32-bit colour sums)
        lf_set_error(h, LF_ERR_UNSUPPORTED, "lf_ai_transform_batch: a strip of %lld points (more than 2^24) is not supported", n);
        return LF_ERR_UNSUPPORTED;
    }
    LF_HIP_CHECK(h, hipSetDevice(h->device));
    hipStream_t s = h->stream;
    const size_t strip_bytes = (size_t)n * 3, frame_bytes = (size_t)rows * cols * 3, fits = 2 * (size_t)n_frames;
    int rc;
    // per fit: 16 f64 (centres, inertia) | 4 counts | 1 status word
    if ((rc = scratch(h, h->ai_lab, fits * (size_t)n)) || (rc = scratch(h, h->ai_fit, fits * (16 * sizeof(double) + 4 * sizeof(long long) + sizeof(int)))) ||
        (rc = scratch(h, h->ai_out, (size_t)n_frames * sizeof(lf_ai_transform)))) return rc;
    const uint8_t* strips;
    long long stride;
    if (frames_on_device) {
        strips = frames + (frame_bytes - strip_bytes);
        stride = (long long)frame_bytes;
    } else {
        // only the strip rows travel: one 2-D copy of n_frames rows of strip_bytes
        if ((rc = scratch(h, h->ai_strip, (size_t)n_frames * strip_bytes)) != LF_OK) return rc;
        LF_HIP_CHECK(h, hipMemcpy2DAsync(h->ai_strip.p, strip_bytes, frames + (frame_bytes - strip_bytes), frame_bytes, strip_bytes, n_frames,
                                         hipMemcpyHostToDevice, s));
        strips = static_cast<const uint8_t*>(h->ai_strip.p);
        stride = (long long)strip_bytes;
    }
    double* fo = static_cast<double*>(h->ai_fit.p);
    long long* fc = reinterpret_cast<long long*>(fo + 16 * fits);
    int* fs = reinterpret_cast<int*>(fc + 4 * fits);
    launch_ai_transform(strips, stride, n_frames, S, cols, static_cast<uint8_t*>(h->ai_lab.p), fo, fc, fs,
                        static_cast<lf_ai_transform*>(h->ai_out.p), s);
    LF_HIP_CHECK(h, hipGetLastError());
    return fetch(h, { { out, h->ai_out.p, (size_t)n_frames * sizeof(lf_ai_transform) } });
}

extern "C" int lf_set_ai_transform(lf_handle* h, const double scale[3], const double shift[3])
{
    if (!h) return LF_ERR_NOT_INITIALISED;
    if (!scale || !shift) { lf_set_error(h, LF_ERR_BAD_ARG, "lf_set_ai_transform: null argument"); return LF_ERR_BAD_ARG; }
    if (const int rc = refuse_in_flight(h)) return rc;
    float sc[3], sh[3];
    for (int i = 0; i < 3; ++i) {
        sc[i] = (float)scale[i]; sh[i] = (float)shift[i];          // scaleandshift2 casts each value to float32 (scale_and_shift.py:28-29)
        if (!isfinite(sc[i]) || !isfinite(sh[i])) {
            lf_set_error(h, LF_ERR_BAD_ARG, "lf_set_ai_transform: scale / shift must be finite as float32");
            return LF_ERR_BAD_ARG;
        }
    }
    // k_pre takes its PreParams by value at each launch: the change applies from the next batch / lf_set_image on
    int identity = 1;
    for (int i = 0; i < 3; ++i) {
        h->cfg.ai_scale[i] = sc[i]; h->cfg.ai_shift[i] = sh[i];
        h->pre.ai_scale[i] = sc[i]; h->pre.ai_shift[i] = sh[i];
        if (sc[i] != 1.f || sh[i] != 0.f) identity = 0;
    }
    h->pre.identity_ai = identity;
    return LF_OK;
}

extern "C" int lf_get_ai_transform(const lf_handle* h, double scale[3], double shift[3])
{
    if (!h) return LF_ERR_NOT_INITIALISED;
    if (!scale || !shift) return LF_ERR_BAD_ARG;
    for (int i = 0; i < 3; ++i) { scale[i] = h->cfg.ai_scale[i]; shift[i] = h->cfg.ai_shift[i]; }
    return LF_OK;
}

// anti-instagram colour clustering (k_kmeans.hip): kmeans.py:22-47
extern "C" int lf_kmeans(lf_handle* h, const uint8_t* bgr_points, int n, int on_device, int k, const double* init_centers, int max_iter,
                         double tol, double* centers_out, long long* counts_out, double* inertia_out, int* n_iter_out)
{
    if (!h) return LF_ERR_NOT_INITIALISED;
    if (!bgr_points || !init_centers || !centers_out || !counts_out || n < 1 || k < 1 || k > 16 || max_iter < 1) {
        lf_set_error(h, LF_ERR_BAD_ARG, "lf_kmeans: null argument, n < 1, max_iter < 1 or k outside 1..16");
        return LF_ERR_BAD_ARG;
    }
    if (n > (1 << 24)) {      // k_kmeans' per-wave 32-bit colour sums (64 lanes x n / 1024 points x 255) stay exact up to here
        lf_set_error(h, LF_ERR_UNSUPPORTED, "lf_kmeans: more than 2^24 points (%d) are not supported", n);
        return LF_ERR_UNSUPPORTED;
    }
    LF_HIP_CHECK(h, hipSetDevice(h->device));
    hipStream_t s = h->stream;
    int rc;
    // f64 scratch: [0 .. 3k) init, [64 .. 64 + 3k] centres + inertia; counts: [k] + the status word behind them
    if ((rc = scratch(h, h->km_lab, (size_t)n)) || (rc = scratch(h, h->km_f64, 128 * sizeof(double))) || (rc = scratch(h, h->km_cnt, 32 * sizeof(long long)))) return rc;
    Staging st(h);
    const uint8_t* dp = st.in(on_device, bgr_points, (size_t)n * 3, h->km_pts);
    st.in(0, init_centers, (size_t)k * 3 * sizeof(double), h->km_f64);
    if ((rc = st.upload()) != LF_OK) return rc;
    double* f64 = static_cast<double*>(h->km_f64.p);
    long long* cnt = static_cast<long long*>(h->km_cnt.p);
    int* status = reinterpret_cast<int*>(cnt + 16);
    launch_kmeans(dp, n, k, f64, max_iter, tol, static_cast<uint8_t*>(h->km_lab.p), f64 + 64, cnt, status, s);
    LF_HIP_CHECK(h, hipGetLastError());
    double res[49];
    long long hc[17];
    if ((rc = fetch(h, { { res, f64 + 64, (size_t)(3 * k + 1) * sizeof(double) }, { hc, cnt, 17 * sizeof(long long) } })) != LF_OK) return rc;
    const int iters = *reinterpret_cast<int*>(&hc[16]);
    if (iters < 0) { lf_set_error(h, LF_ERR_BAD_ARG, "lf_kmeans: a cluster stayed empty (fewer distinct samples than clusters)"); return LF_ERR_BAD_ARG; }
    for (int j = 0; j < 3 * k; ++j) centers_out[j] = res[j];
    for (int j = 0; j < k; ++j) counts_out[j] = hc[j];
    if (inertia_out) *inertia_out = res[3 * k];
    if (n_iter_out) *n_iter_out = iters;
    return LF_OK;
}
