// Host side of LF_DETECTOR_DENSE: the parameter (lf_dense_*) and the buffers of k_pre<true> / k_dense, sized once per handle.
#include <math.h>
#include "lanefront_handle.h"

using namespace lf;

extern "C" void lf_dense_default_params(lf_dense_params* p)
{
    if (!p) return;
    p->sobel_threshold = 40.0;          // default_ld2.yaml of line_detector_node
}

extern "C" int lf_set_dense_params(lf_handle* h, const lf_dense_params* p)
{
    if (!h) return LF_ERR_NOT_INITIALISED;
    if (!p) { lf_set_error(h, LF_ERR_BAD_ARG, "lf_set_dense_params: null params"); return LF_ERR_BAD_ARG; }
    if (const int rc = refuse_in_flight(h)) return rc;
    if (!(p->sobel_threshold >= 0)) {
        lf_set_error(h, LF_ERR_BAD_ARG, "lf_set_dense_params: sobel_threshold %g must be a number >= 0", p->sobel_threshold);
        return LF_ERR_BAD_ARG;
    }
    h->dense_params = *p;
    return LF_OK;
}

extern "C" int lf_get_dense_params(const lf_handle* h, lf_dense_params* p)
{
    if (!h) return LF_ERR_NOT_INITIALISED;
    if (!p) return LF_ERR_BAD_ARG;
    *p = h->dense_params;
    return LF_OK;
}

// the undilated mask planes and the per-slot (normal, pixel) records of every problem (once per handle; lf_set_detector)
int lf::dense_prepare(lf_handle* h)
{
    if (h->Hc < 3 || h->W < 3) {
        lf_set_error(h, LF_ERR_UNSUPPORTED, "LF_DETECTOR_DENSE: a %dx%d working image is below the 5x5 Sobel's 3 pixels a side", h->Hc, h->W);
        return LF_ERR_UNSUPPORTED;
    }
    if (h->d_bwbits && h->d_dense_rec) return LF_OK;
    LF_HIP_CHECK(h, hipSetDevice(h->device));
    const size_t nprob = (size_t)h->max_frames * 3;
    if (dalloc(h, &h->d_bwbits, nprob * h->Hc * h->Ww) || dalloc(h, &h->d_dense_rec, nprob * (size_t)h->cap_lines * 4)) {
        h->d_bwbits.reset(); h->d_dense_rec.reset();
        return LF_ERR_HIP;
    }
    return LF_OK;
}
