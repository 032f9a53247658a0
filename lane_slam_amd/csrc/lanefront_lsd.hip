// lf::LsdState (lanefront_handle.h): the LSD detector's parameters, tables and device arrays, the growth of its lists, and the stage
// calls that wire those arrays into the launchers of k_lsd_grad / order / seed32 / label / grow.  Host code only.
#include <string.h>
#include <math.h>
#include <vector>
#include "lanefront_handle.h"
#include "lsd_bitplane.h"
#include "k_lsd_grad.h"

namespace lf {

// LsdState::d_zero for nprob problems, d_maxgrad | d_nrec | d_nlow | d_tile_count [4] | status: the byte offsets of its parts
struct CounterBlock {
    size_t nrec, nlow, tile_count, status, bytes;
    explicit CounterBlock(size_t nprob) : nrec(nprob * 8), nlow(nrec + nprob * 4), tile_count(nlow + nprob * 4), status(tile_count + 16), bytes(status + sizeof(BatchStatus)) {}
};

int LsdState::init(lf_handle* h, int Hc, int W, const lf_lsd_options& o, int seed_order_, int max_frames_, int cap_lines)
{
    seed_order = seed_order_;
    max_frames = max_frames_;
    // ---- parameters
    LsdParams& L = params;
    memset(&L, 0, sizeof(L));
    L.Hc = Hc; L.W = W; L.Ww = (W + 31) / 32;
    L.scaled = o.scale != 1.0;
    L.scale = o.scale;
    if (o.scale <= 0 || o.scale > 1.0) { lf_set_error(h, LF_ERR_UNSUPPORTED, "lsd_scale must be in (0,1]"); return LF_ERR_UNSUPPORTED; }
    if (L.scaled) { L.Ws = dm::round_half_even(W * o.scale); L.Hs = dm::round_half_even(Hc * o.scale); }
    else { L.Ws = W; L.Hs = Hc; }
    const int Hs = L.Hs, Ws = L.Ws;
    Ps = (size_t)Hs * Ws;
    if (Ps >= (1u << 20) || L.Ws > 65535 || L.Hs > 65535) { lf_set_error(h, LF_ERR_UNSUPPORTED, "scaled LSD image too large"); return LF_ERR_UNSUPPORTED; }
    // LDS limit of region growing, checked once here so that an unsupported geometry fails at creation instead of as a launch error
    // later: it keeps the row-start table of its problem in LDS (k_lsd_grow.hip)
    if ((size_t)((L.Hs + 2) & ~1) * 4 + 512 * 4 + 1024 > 64 * 1024) { lf_set_error(h, LF_ERR_UNSUPPORTED, "scaled LSD image has %d rows: the row table exceeds the LDS of one problem", L.Hs); return LF_ERR_UNSUPPORTED; }
    if (o.n_bins < 2 || o.n_bins > 4096) { lf_set_error(h, LF_ERR_UNSUPPORTED, "lsd_n_bins must be in [2,4096] (a seed is its bin above a 20-bit pixel index in one word)"); return LF_ERR_UNSUPPORTED; }
    if (L.scaled) {
        const double sigma = (o.scale < 1) ? (o.sigma_scale / o.scale) : o.sigma_scale;
        const double sprec = 3;
        const unsigned hh = (unsigned)ceil(sigma * sqrt(2 * sprec * dm::dlog(10.0)));
        const int n = 1 + 2 * (int)hh;
        if (n > kMaxGaussTaps) { lf_set_error(h, LF_ERR_UNSUPPORTED, "LSD Gaussian needs %d taps (max %d)", n, kMaxGaussTaps); return LF_ERR_UNSUPPORTED; }
        const double scale2X = -0.5 / (sigma * sigma);
        double sum = 0;
        for (int i = 0; i < n; ++i) { double x = i - (n - 1) * 0.5; double t = dm::dexp(scale2X * x * x); L.k[i] = t; sum += t; }
        sum = 1.0 / sum;
        for (int i = 0; i < n; ++i) L.k[i] *= sum;
        L.ntaps = n; L.half = n / 2;
    } else { L.ntaps = 1; L.half = 0; L.k[0] = 1.0; }
    L.prec = 3.14159265358979323846 * o.ang_th / 180;
    L.p = o.ang_th / 180;
    L.rho = o.quant / dm::dsin(L.prec);
    L.log_nt = 5 * (dm::dlog10((double)L.Ws) + dm::dlog10((double)L.Hs)) / 2 + dm::dlog10(11.0);
    L.min_reg_size = (int)(-L.log_nt / dm::dlog10(L.p));
    L.log_eps = o.log_eps; L.density_th = o.density_th;
    L.n_bins = o.n_bins; L.refine = o.refine; L.cap_lines = cap_lines;
    if (seed_order != LF_LSD_SEED_OPENCV30 && seed_order != LF_LSD_SEED_OPENCV32) { lf_set_error(h, LF_ERR_BAD_ARG, "lsd_seed_order %d: LF_LSD_SEED_OPENCV30 or LF_LSD_SEED_OPENCV32", seed_order); return LF_ERR_BAD_ARG; }
    if (seed_order == LF_LSD_SEED_OPENCV32 && !lsd_seed32_supported(L)) { lf_set_error(h, LF_ERR_UNSUPPORTED, "lsd_seed_order OPENCV32: the %dx%d LSD image exceeds the row tables of the sort emulation, or (n_bins - 1) * quant / sin(ang_th) < 361 (k_lsd_seed32.hip)", L.Ws, L.Hs); return LF_ERR_UNSUPPORTED; }
    // component labelling (k_lsd_label): problems of up to label_lds = 6144 defined pixels in LDS (24 KB per workgroup: what one
    // workgroup of k_lsd_grow gives back when it leaves a CU), the larger ones in the problem's region scratch, up to label_items
    // -- a third of the scaled image (every growing wave has a region list of that size in the scratch) and below 2^16 (the
    // labels are u16).  Rounds 2 - 3 had every problem's tables in LDS, 48 KB per workgroup growing with the workload to 144 KB.
    L.label_lds = kLabelLds;
    {
        // images whose bit plane is larger than that anyway (1080p: 124 KB, one workgroup per CU): the LDS form for every problem
        // that fits the same request
        const size_t plane = bitplane_lds_words(Ps) * 4;
        if (plane <= 150 * 1024 && plane / 4 > (size_t)L.label_lds) L.label_lds = (int)((plane / 4 < 65534 ? plane / 4 : 65534) & ~(size_t)1);
    }
    L.label_items = (int)(Ps / 3 / 1024) * 1024;
    if (L.label_items > 64512) L.label_items = 64512;
    if (L.label_items < kLabelItems) L.label_items = kLabelItems;
    L.label_items_max = L.label_items;
    label_items_full = L.label_items;
    L.rec_cap = (int)Ps;                               // (alloc_lists sets the capacity its caller chooses)
    // ---- resize tables (cv::resize INTER_LINEAR, CV_64F)
    std::vector<int> xofs(Ws), y0(Hs), y1(Hs);
    std::vector<float> xa(2 * (size_t)Ws), yb(2 * (size_t)Hs);
    int xmax = Ws;
    const double scale_x = 1.0 / L.scale, scale_y = 1.0 / L.scale;
    for (int dx = 0; dx < Ws; ++dx) {
        float fx; int sx;
        if (L.scaled) {
            fx = (float)((dx + 0.5) * scale_x - 0.5);
            sx = dm::ifloor((double)fx);
            fx -= sx;
        } else { fx = 0.f; sx = dx; }
        if (sx < 0) { fx = 0; sx = 0; }
        if (sx + 1 >= W) {
            if (dx < xmax) xmax = dx;
            if (sx >= W - 1) { fx = 0; sx = W - 1; }
        }
        xofs[dx] = sx; xa[2 * dx] = 1.f - fx; xa[2 * dx + 1] = fx;
    }
    for (int dy = 0; dy < Hs; ++dy) {
        float fy; int sy;
        if (L.scaled) {
            fy = (float)((dy + 0.5) * scale_y - 0.5);
            sy = dm::ifloor((double)fy);
            fy -= sy;
        } else { fy = 0.f; sy = dy; }
        yb[2 * dy] = 1.f - fy; yb[2 * dy + 1] = fy;
        y0[dy] = sy < 0 ? 0 : (sy > Hc - 1 ? Hc - 1 : sy);
        y1[dy] = sy + 1 < 0 ? 0 : (sy + 1 > Hc - 1 ? Hc - 1 : sy + 1);
    }
    // the tiles of k_lsd_grad (k_lsd_grad.h): the worst one's raw footprint, its wave's LDS slice, what a list entry can name
    lsd_grad_footprint(xofs.data(), y0.data(), y1.data(), W, Ws, Hs, &max_nsx, &max_nsy);
    {
        const size_t lds = lsd_grad_carve(L.half, max_nsx, max_nsy).bytes + kLsdGradStaticLds;
        if (lds > kLsdGradMaxLds) { lf_set_error(h, LF_ERR_UNSUPPORTED, "lsd_scale %.3f needs %zu B of LDS per tile (max %zu)", L.scale, lds, kLsdGradMaxLds); return LF_ERR_UNSUPPORTED; }
        if (lsd_tiles_x(Ws) > kLsdMaxTilesPerSide || lsd_tiles_y(Hs) > kLsdMaxTilesPerSide || max_frames * 3 > kLsdMaxTileProblems || L.Ww > kLsdMaxWordCols) {
            lf_set_error(h, LF_ERR_UNSUPPORTED, "LSD image %d x %d of %d frames: more tiles than a tile list entry names", Ws, Hs, max_frames);
            return LF_ERR_UNSUPPORTED;
        }
    }
    if (dalloc(h, &d_xofs, Ws) || dalloc(h, &d_y0, Hs) || dalloc(h, &d_y1, Hs) || dalloc(h, &d_xa, 2 * (size_t)Ws) || dalloc(h, &d_yb, 2 * (size_t)Hs))
        return LF_ERR_HIP;
    LF_HIP_CHECK(h, hipMemcpy(d_xofs, xofs.data(), Ws * sizeof(int), hipMemcpyHostToDevice));
    LF_HIP_CHECK(h, hipMemcpy(d_y0, y0.data(), Hs * sizeof(int), hipMemcpyHostToDevice));
    LF_HIP_CHECK(h, hipMemcpy(d_y1, y1.data(), Hs * sizeof(int), hipMemcpyHostToDevice));
    LF_HIP_CHECK(h, hipMemcpy(d_xa, xa.data(), 2 * (size_t)Ws * sizeof(float), hipMemcpyHostToDevice));
    LF_HIP_CHECK(h, hipMemcpy(d_yb, yb.data(), 2 * (size_t)Hs * sizeof(float), hipMemcpyHostToDevice));
    rt.xofs = d_xofs; rt.xa = d_xa; rt.y0 = d_y0; rt.y1 = d_y1; rt.yb = d_yb; rt.xmax = xmax;
    // ---- the fixed per-problem arrays
    const size_t nprob = (size_t)max_frames * 3, cap = nprob * (size_t)cap_lines;
    if (dalloc(h, &d_tile_list, nprob * (size_t)(lsd_tiles_x(Ws) * lsd_tiles_y(Hs))) ||
        dalloc(h, &d_gused, nprob * ((Ps + 31) / 32)) || dalloc(h, &d_row_start, nprob * (size_t)(Hs + 1)) ||
        dalloc(h, &d_comp_list, nprob * (size_t)kCompCap) || dalloc(h, &d_comp_count, nprob) || dalloc(h, &d_perm, nprob) || dalloc(h, &d_comp_key, nprob) ||
        dalloc(h, &d_tmp_lines, cap * 4) || dalloc(h, &d_tmp_tags, cap) || dalloc(h, &d_norder, nprob))
        return LF_ERR_HIP;
    // ---- the counter block, zeroed once here
    const CounterBlock cb(nprob);
    zero_bytes = cb.bytes;
    if (dalloc(h, &d_zero, zero_bytes)) return LF_ERR_HIP;
    d_maxgrad = reinterpret_cast<unsigned long long*>(d_zero.p);
    d_nrec = reinterpret_cast<int*>(d_zero + cb.nrec);
    if (seed_order == LF_LSD_SEED_OPENCV32) d_nlow = reinterpret_cast<int*>(d_zero + cb.nlow);
    d_tile_count = reinterpret_cast<int*>(d_zero + cb.tile_count);
    d_status = reinterpret_cast<BatchStatus*>(d_zero + cb.status);
    LF_HIP_CHECK(h, hipMemset(d_zero, 0, zero_bytes));
    // ---- test and tuning overrides of k_lsd_grow, clamped
    if (const char* ev = getenv("LF_GROW_LDS_LEVEL")) { const int v = atoi(ev); env_lds_level = v < 0 ? 0 : (v > 2 ? 2 : v); }
    if (const char* ev = getenv("LF_GROW_MIXED")) env_mixed = atoi(ev) != 0 ? 1 : 0;
    if (const char* ev = getenv("LF_GROW_BITMAP")) { const int v = atoi(ev); env_bitmap = v < 0 ? 0 : v; }       // > 1: that many USED bits (tests)
    return LF_OK;
}

void LsdState::free_lists()
{
    for (auto* b : { &d_raddr, &d_order_a, &d_order_b, &d_cxy, &d_reg, &d_laddr }) b->reset();
    for (auto* b : { &d_rdeg, &d_cdeg, &d_rsd, &d_csd }) b->reset();
    for (auto* b : { &d_rmod, &d_rcs, &d_rsn, &d_cmod, &d_ccs, &d_lmod }) b->reset();
    d_sort_a.reset(); d_sort_b.reset(); d_clabel.reset();
    params.r_sd = nullptr; params.c_sd = nullptr;
}

int LsdState::alloc_lists(lf_handle* h, int rec_cap)
{
    const size_t nprob = (size_t)max_frames * 3, S = (size_t)rec_cap;
    LsdParams& L = params;
    L.rec_cap = rec_cap;
    // (components are only kept apart for problems of up to label_items defined pixels; no problem has more than rec_cap)
    // (... but not below kLabelItems: the labelling kernel's LDS form and the growing waves' scratch slices are laid out for that)
    const int li = rec_cap > kLabelItems ? rec_cap : kLabelItems;
    L.label_items = label_items_full < li ? label_items_full : li;
    L.label_items_max = L.label_items;
    if (dalloc(h, &d_raddr, nprob * S) || dalloc(h, &d_rdeg, nprob * S) || dalloc(h, &d_rmod, nprob * S) ||
        dalloc(h, &d_rcs, nprob * S) || dalloc(h, &d_rsn, nprob * S) || dalloc(h, &d_sort_a, nprob * S) || dalloc(h, &d_sort_b, nprob * S) ||
        dalloc(h, &d_order_a, nprob * S) || dalloc(h, &d_order_b, nprob * S) || dalloc(h, &d_cxy, nprob * S) || dalloc(h, &d_cdeg, nprob * S) ||
        dalloc(h, &d_cmod, nprob * S) || dalloc(h, &d_ccs, nprob * S * 2) || dalloc(h, &d_reg, nprob * lsd_grow_reg_stride(L)) ||
        dalloc(h, &d_clabel, nprob * S))
        return LF_ERR_HIP;
    if (dalloc(h, &d_rsd, nprob * S * 2) || dalloc(h, &d_csd, nprob * S * 2)) return LF_ERR_HIP;
    L.r_sd = d_rsd; L.c_sd = d_csd;
    if (seed_order == LF_LSD_SEED_OPENCV32 && (dalloc(h, &d_laddr, nprob * S) || dalloc(h, &d_lmod, nprob * S)))
        return LF_ERR_HIP;
    return LF_OK;
}

// The per-problem lists of the LSD stages hold LsdParams::rec_cap entries.  When a batch had a problem with more (BatchStatus::rec_need, read
// by the caller: the largest need), that problem was dropped on the device; here the lists are reallocated with room to spare and the
// caller runs the batch again.  The stream must be idle.  Results never depend on the capacity -- only whether a batch runs twice.
int LsdState::grow_lists(lf_handle* h, int need)
{
    size_t cap = ((size_t)need + (size_t)need / 4 + 4095) / 4096 * 4096;
    if (cap > Ps) cap = Ps;
    if (alloc_trace()) fprintf(stderr, "lanefront: a problem needs %d list entries, the handle holds %d: growing to %zu\n", need, params.rec_cap, cap);
    const int old_cap = params.rec_cap;
    free_lists();
    int rc = alloc_lists(h, (int)cap);
    if (rc == LF_OK) { ++lists_grown; lists_lost = false; return LF_OK; }
    // Out of memory part way: never leave the handle with null lists behind a capacity that says otherwise (the next batch would launch
    // the LSD kernels on them -- a GPU fault, not an error code).  Back to the capacity that did fit; when even that fails now, the
    // handle refuses every later detect call (lists_lost) until a growth succeeds.
    free_lists();
    if (alloc_lists(h, old_cap) != LF_OK) { free_lists(); params.rec_cap = old_cap; lists_lost = true; }
    lf_set_error(h, LF_ERR_HIP, "out of device memory growing the LSD lists from %d to %zu entries per problem%s", old_cap, cap,
                 lists_lost ? "; the lists are gone: the handle refuses detection" : "; the handle keeps its old lists");
    return LF_ERR_HIP;
}

// The next batch's region-growing slices (performance only: the results do not depend on them): 13 KB while nearly every
// problem fits it (the synthetic lane frames), 28 KB when more than 5 % overflow it (real camera frames have two to three
// times the edge pixels), 40 KB when more than 25 % overflow 28 KB.
void LsdState::adapt_slice(int over_small, int over_medium, int problems)
{
    grow_lds_level = over_medium * 4 > problems ? 2 : (over_small * 20 > problems ? 1 : 0);
    grow_mixed = (grow_lds_level == 0 ? over_small : over_medium) * 100 > problems;
}

// The views of the arrays above (common.h): every owner is named in one of them and nowhere else below
LsdRecords LsdState::records() const
{
    LsdRecords v{};
    v.r_addr = d_raddr; v.r_deg = d_rdeg; v.r_mod = d_rmod; v.r_cs = d_rcs; v.r_sn = d_rsn;
    v.n_rec = d_nrec; v.maxgrad = d_maxgrad;
    v.l_addr = d_laddr; v.l_mod = d_lmod; v.n_low = d_nlow;
    v.list = d_tile_list; v.list_count = d_tile_count;
    v.max_nsx = max_nsx; v.max_nsy = max_nsy;
    return v;
}

LsdCompact LsdState::compact() const
{
    LsdCompact v{};
    v.sort_a = d_sort_a; v.sort_b = d_sort_b; v.order_a = d_order_a; v.order_b = d_order_b;
    v.norder = d_norder;
    v.c_xy = d_cxy; v.c_deg = d_cdeg; v.c_mod = d_cmod;
    v.c_cs = d_ccs; v.c_sn = d_ccs ? d_ccs + 1 : nullptr;        // (cos, sin) pairs in one array: k_lsd_order.hip
    v.row_start = d_row_start;
    return v;
}

LsdComponents LsdState::components(bool use_perm) const
{
    LsdComponents v{};
    v.c_label = d_clabel;
    v.comp_list = d_comp_list; v.comp_count = d_comp_count; v.comp_key = d_comp_key; v.comp_cap = kCompCap;
    v.perm = use_perm ? d_perm.p : nullptr;
    v.reg = d_reg; v.gused = d_gused;
    v.tmp_lines = d_tmp_lines; v.tmp_tags = d_tmp_tags;
    return v;
}

void LsdState::grad(int n, const uint32_t* edge_bits, const uint32_t* mask_bits, bool counters_zeroed, hipStream_t s)
{
    launch_lsd_grad(params, rt, records(), n, edge_bits, mask_bits, &d_status->rec_need, counters_zeroed, s);
}

void LsdState::grad_gray(int n, const uint8_t* gray, hipStream_t s)
{
    launch_lsd_grad_gray(params, rt, records(), n, gray, s);
}

void LsdState::order(int n, int big, hipStream_t s)
{
    launch_lsd_order(params, records(), compact(), n, s);
    // OpenCV >= 3.2: the seeds in the order std::sort leaves them in (the compact arrays and row starts stay as they are)
    if (seed_order == LF_LSD_SEED_OPENCV32) launch_lsd_seed32(params, records(), compact(), n, &d_status->rec_need, big, s);
}

void LsdState::label(int n, bool rank, hipStream_t s)
{
    launch_lsd_label(params, compact(), components(), n, s);
    if (rank) launch_lsd_rank(components(), n * 3, s);
}

void LsdState::grow(int n, float* lines, int* counts, int lds_kb, bool mixed, bool use_perm, hipStream_t s)
{
    launch_lsd_grow(params, compact(), components(use_perm), n, lines, counts, lds_kb, mixed, env_bitmap, s);
}

}  // namespace lf
