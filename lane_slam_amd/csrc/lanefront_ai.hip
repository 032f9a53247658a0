// Host side of the anti-instagram estimate (k_ai.hip) and the setter of the transform k_pre applies.
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
    if (h->pending) { lf_set_error(h, LF_ERR_BAD_ARG, "a batch is in flight on this handle: call lf_wait first"); return LF_ERR_BAD_ARG; }
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
    LF_HIP_CHECK(h, hipMemcpyAsync(out, h->ai_out.p, (size_t)n_frames * sizeof(lf_ai_transform), hipMemcpyDeviceToHost, s));
    LF_HIP_CHECK(h, hipStreamSynchronize(s));
    return LF_OK;
}

extern "C" int lf_set_ai_transform(lf_handle* h, const double scale[3], const double shift[3])
{
    if (!h) return LF_ERR_NOT_INITIALISED;
    if (!scale || !shift) { lf_set_error(h, LF_ERR_BAD_ARG, "lf_set_ai_transform: null argument"); return LF_ERR_BAD_ARG; }
    if (h->pending) { lf_set_error(h, LF_ERR_BAD_ARG, "a batch is in flight on this handle: call lf_wait first"); return LF_ERR_BAD_ARG; }
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
