// Host side of LF_DETECTOR_HOUGH: the parameters (lf_hough_*), the tables and scratch of k_hough, sized once per handle.
#include <string.h>
#include "lanefront_handle.h"

using namespace lf;

static bool hough_params_ok(const lf_hough_params& P)
{
    return P.threshold >= 1 && P.min_line_length >= 0 && P.max_line_gap >= 0;
}

// HoughLinesP takes float rho and theta: a double that rounds to the same floats computes the same lines
static bool hough_params_supported(const lf_hough_params& P)
{
    return (float)P.rho == 1.f && (float)P.theta == (float)(3.14159265358979323846 / 180);
}

extern "C" void lf_hough_default_params(lf_hough_params* p)
{
    if (!p) return;
    p->threshold = 2; p->min_line_length = 3; p->max_line_gap = 1;         // default.yaml of line_detector_node
    p->rho = 1.0; p->theta = 3.14159265358979323846 / 180;
}

extern "C" int lf_set_hough_params(lf_handle* h, const lf_hough_params* p)
{
    if (!h) return LF_ERR_NOT_INITIALISED;
    if (!p) { lf_set_error(h, LF_ERR_BAD_ARG, "lf_set_hough_params: null params"); return LF_ERR_BAD_ARG; }
    if (const int rc = refuse_in_flight(h)) return rc;
    if (!hough_params_ok(*p)) {
        lf_set_error(h, LF_ERR_BAD_ARG, "lf_set_hough_params: threshold %d must be >= 1, min_line_length %d and max_line_gap %d >= 0",
                     p->threshold, p->min_line_length, p->max_line_gap);
        return LF_ERR_BAD_ARG;
    }
    if (!hough_params_supported(*p)) {
        lf_set_error(h, LF_ERR_UNSUPPORTED, "lf_set_hough_params: rho %g, theta %g: only rho 1 and theta pi/180 are supported", p->rho, p->theta);
        return LF_ERR_UNSUPPORTED;
    }
    h->hough_params = *p;
    return LF_OK;
}

extern "C" int lf_get_hough_params(const lf_handle* h, lf_hough_params* p)
{
    if (!h) return LF_ERR_NOT_INITIALISED;
    if (!p) return LF_ERR_BAD_ARG;
    *p = h->hough_params;
    return LF_OK;
}

// the tables of the handle's geometry and the scratch of every resident workgroup (once per handle; lf_set_detector)
int lf::hough_prepare(lf_handle* h)
{
    int lds_points = 0;
    const size_t lds = hough_lds_bytes(h->Hc, h->W, &lds_points);
    if (!lds) {
        lf_set_error(h, LF_ERR_UNSUPPORTED, "LF_DETECTOR_HOUGH: a %dx%d working image is beyond k_hough (at most %d a side, edge bit plane <= 48 KB)",
                     h->Hc, h->W, kHoughMaxSide);
        return LF_ERR_UNSUPPORTED;
    }
    if (h->d_hough_tab) return LF_OK;
    LF_HIP_CHECK(h, hipSetDevice(h->device));
    HoughTables t;
    hough_tables(h->Hc, h->W, t);
    // as many workgroups as fit the device at once (LDS bounds them), never more than the problems of a batch
    int cus = 0;
    LF_HIP_CHECK(h, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->device));
    const int per_cu = (int)((160 * 1024) / lds);
    int slots = (cus > 0 ? cus : 1) * (per_cu > 0 ? per_cu : 1);
    if (slots > h->max_frames * 3) slots = h->max_frames * 3;
    if (slots > 1024) slots = 1024;
    HoughParams& hp = h->hough_p;
    hp.Hc = h->Hc; hp.W = h->W; hp.Ww = h->Ww;
    hp.cap_lines = h->cap_lines;
    hp.cells = t.off[kHoughAngles];
    hp.lds_points = lds_points;
    hp.nz_stride = (size_t)lds_points < (size_t)h->Hc * h->W ? (size_t)h->Hc * h->W : 0;
    if (dalloc(h, &h->d_hough_acc, (size_t)slots * hp.cells) || (hp.nz_stride && dalloc(h, &h->d_hough_nz, (size_t)slots * hp.nz_stride)) ||
        dalloc(h, &h->d_hough_tab, 1)) {
        h->d_hough_acc.reset(); h->d_hough_nz.reset(); h->d_hough_tab.reset();
        return LF_ERR_HIP;
    }
    LF_HIP_CHECK(h, hipMemcpy(h->d_hough_tab, &t, sizeof(t), hipMemcpyHostToDevice));
    h->hough_slots = slots;
    return LF_OK;
}
