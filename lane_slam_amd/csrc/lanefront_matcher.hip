// BinaryDescriptorMatcher's DATASET form (round 5): descriptors of several train images are
// added one Mat at a time, searched as ONE set, and every match says which image it came from.
//   ref: src/line_descriptor/src/binary_descriptor_matcher.cpp
//     :70-80    add      descriptorsMat.push_back(descriptors[i]); indexesMap[nextAddedIndex] = numImages; nextAddedIndex += rows
//     :83-93    train    the Mihasher is populated with all rows (rebuilt from everything added so far)
//     :96-104   clear
//     :117-195  match    K = 1 over the whole set; imgIdx = the image whose rows hold the result (indexesMap.upper_bound - 1),
//                        trainIdx = the row number IN THE SET (results - 1: not rebased to the image), and masks[imgIdx][query] == 0
//                        drops the DMatch AFTER the search (it does not steer it)
//     :339-425  knnMatch the same per result, lists per query, compactResult drops empty lists
//     :508-595  radiusMatch  K = all, results with distance <= maxDistance, same image lookup / mask / compactResult
// The searches are this library's own (lf_associate / lf_knn_match / lf_radius_match on the concatenated codes, with the
// handle's tie rule); what is added here is the set, the image lookup and the mask rule.
// The pair forms the set is searched with live here as well, in front of it: lf_associate (k_assoc.hip, k_assoc_ties.hip) with its
// tie rule, lf_associate_float, and lf_select_queries / lf_knn_match / lf_radius_match (k_knn.hip).

#include <string.h>
#include <algorithm>
#include <functional>
#include "lanefront_handle.h"

using namespace lf;

// ---------------------------------------------------------------------------------------- the pair forms
extern "C" int lf_associate(lf_handle* h, const uint8_t* query32, int nq, const uint8_t* map32, int nm,
                            int32_t* idx, float* dist, int on_device)
{
    if (!h) return LF_ERR_NOT_INITIALISED;
    if (nq < 0 || nm < 0 || (nq > 0 && (!query32 || !idx || !dist)) || (nm > 0 && !map32)) { lf_set_error(h, LF_ERR_BAD_ARG, "lf_associate: bad argument"); return LF_ERR_BAD_ARG; }
    if (nm > (1 << 21)) { lf_set_error(h, LF_ERR_UNSUPPORTED, "map larger than 2^21 entries"); return LF_ERR_UNSUPPORTED; }
    if (nq == 0) return LF_OK;
    // the tie pass has room for 1023 blocks of 256 queries (k_assoc_ties.hip); refused here, before anything is queued
    if (h->tie_rule == LF_TIE_MIHASHER && nm > 0 && !assoc_ties_fit(assoc_plan(nq, nm))) {
        lf_set_error(h, LF_ERR_UNSUPPORTED, "lf_associate: %d queries are more than the tie pass of LF_TIE_MIHASHER takes (261888): split the batch or use LF_TIE_LOWEST", nq);
        return LF_ERR_UNSUPPORTED;
    }
    LF_HIP_CHECK(h, hipSetDevice(h->device));
    hipStream_t s = h->stream;
    if (nm == 0) {
        // descriptor matrices cannot be void (binary_descriptor_matcher.cpp:201-205): report "no match"
        std::vector<int32_t> hi(nq, -1); std::vector<float> hd(nq, -1.f);
        if (on_device) {
            LF_HIP_CHECK(h, hipMemcpyAsync(idx, hi.data(), nq * sizeof(int32_t), hipMemcpyHostToDevice, s));
            LF_HIP_CHECK(h, hipMemcpyAsync(dist, hd.data(), nq * sizeof(float), hipMemcpyHostToDevice, s));
            LF_HIP_CHECK(h, hipStreamSynchronize(s));
        } else { memcpy(idx, hi.data(), nq * sizeof(int32_t)); memcpy(dist, hd.data(), nq * sizeof(float)); }
        return LF_OK;
    }
    const size_t nm_pad = assoc_rows_padded_m(nm);
    int rc;
    if ((rc = scratch(h, h->a_mx, nm_pad * 256)) != LF_OK) return rc;     // 256 B per 128-B row: the tile loop's LDS-DMA read-ahead is not shown to stay within 128 B x nm_pad
    const bool ties = h->tie_rule == LF_TIE_MIHASHER;
    if (ties && (rc = scratch(h, h->a_best, (size_t)nq * 8)) != LF_OK) return rc;
    Staging st(h);
    const uint8_t* dq = st.in(on_device, query32, (size_t)nq * 32, h->a_q);
    const uint8_t* dmp = st.in(on_device, map32, (size_t)nm * 32, h->a_m);
    int32_t* didx = st.out(on_device, idx, (size_t)nq * 4, h->a_idx);
    float* ddist = st.out(on_device, dist, (size_t)nq * 4, h->a_dist);
    if ((rc = st.upload()) != LF_OK) return rc;
    {
        StageClock::Scope t(h, h->clock, ST_ASSOC);
        h->a_ws.tie_res = ties ? static_cast<unsigned long long*>(h->a_best.p) : nullptr;      // (the distance pass then lists the queries of the tie pass)
        LF_HIP_CHECK(h, launch_assoc(dq, nq, dmp, nm, (int8_t*)h->a_mx.p, h->a_ws, didx, ddist, s));
        if (ties)
            LF_HIP_CHECK(h, launch_assoc_ties(dq, nullptr, nq, (const int8_t*)h->a_mx.p, dmp, nullptr, nm, nullptr, 0, h->a_ws,
                                              static_cast<unsigned long long*>(h->a_best.p), didx, ddist, s));
    }
    LF_HIP_CHECK(h, hipGetLastError());
    return fetch(h, { { idx, didx, (size_t)nq * 4 }, { dist, ddist, (size_t)nq * 4 } });
}

extern "C" int lf_set_tie_rule(lf_handle* h, int tie_rule)
{
    if (!h) return LF_ERR_NOT_INITIALISED;
    if (tie_rule != LF_TIE_LOWEST && tie_rule != LF_TIE_MIHASHER) { lf_set_error(h, LF_ERR_BAD_ARG, "lf_set_tie_rule: unknown rule %d", tie_rule); return LF_ERR_BAD_ARG; }
    h->tie_rule = tie_rule;
    return LF_OK;
}

extern "C" int lf_associate_float(lf_handle* h, const float* query72, int nq, const float* map72, int nm,
                                  int32_t* idx, float* dist, int on_device)
{
    if (!h) return LF_ERR_NOT_INITIALISED;
    if (nq <= 0 || nm <= 0 || !query72 || !map72 || !idx || !dist) { lf_set_error(h, LF_ERR_BAD_ARG, "lf_associate_float: bad argument"); return LF_ERR_BAD_ARG; }
    LF_HIP_CHECK(h, hipSetDevice(h->device));
    hipStream_t s = h->stream;
    int rc;
    if ((rc = scratch(h, h->a_best, assoc_float_scratch_bytes(nq, nm))) || (rc = scratch(h, h->a_qn, (size_t)nq * 4)) || (rc = scratch(h, h->a_mn, (size_t)nm * 4))) return rc;
    Staging st(h);
    const float* dq = st.in(on_device, query72, (size_t)nq * 288, h->a_q);
    const float* dmp = st.in(on_device, map72, (size_t)nm * 288, h->a_m);
    int32_t* didx = st.out(on_device, idx, (size_t)nq * 4, h->a_idx);
    float* ddist = st.out(on_device, dist, (size_t)nq * 4, h->a_dist);
    if ((rc = st.upload()) != LF_OK) return rc;
    {
        StageClock::Scope t(h, h->clock, ST_ASSOC);
        LF_HIP_CHECK(h, launch_assoc_float(dq, nq, dmp, nm, (float*)h->a_qn.p, (float*)h->a_mn.p, h->a_best.p, didx, ddist, s));
    }
    LF_HIP_CHECK(h, hipGetLastError());
    return fetch(h, { { idx, didx, (size_t)nq * 4 }, { dist, ddist, (size_t)nq * 4 } });
}

// knnMatch / radiusMatch (binary_descriptor_matcher.cpp:258-335, 428-504): k_knn.hip
extern "C" int lf_select_queries(lf_handle* h, const uint8_t* query32, int nq, const uint8_t* mask, uint8_t* selected32, int32_t* query_idx,
                                 int* n_selected, int on_device)
{
    if (!h) return LF_ERR_NOT_INITIALISED;
    if (nq < 0 || !n_selected || (nq > 0 && (!query32 || !mask || !selected32 || !query_idx))) { lf_set_error(h, LF_ERR_BAD_ARG, "lf_select_queries: bad argument"); return LF_ERR_BAD_ARG; }
    *n_selected = 0;
    if (nq == 0) return LF_OK;
    LF_HIP_CHECK(h, hipSetDevice(h->device));
    hipStream_t s = h->stream;
    int rc;
    if ((rc = scratch(h, h->kn_total, 4 * sizeof(int))) != LF_OK) return rc;
    Staging st(h);
    const uint8_t* dq = st.in(on_device, query32, (size_t)nq * 32, h->a_q);
    const uint8_t* dmask = st.in(on_device, mask, (size_t)nq, h->a_dist);             // (no distances in this call: their buffer carries the mask)
    uint8_t* dsel = st.out(on_device, selected32, (size_t)nq * 32, h->a_m);
    int32_t* dqi = st.out(on_device, query_idx, (size_t)nq * 4, h->a_idx);
    if ((rc = st.upload()) != LF_OK) return rc;
    launch_select_queries(dq, dmask, nq, dsel, dqi, static_cast<int*>(h->kn_total.p), s);
    LF_HIP_CHECK(h, hipGetLastError());
    int n = 0;
    if ((rc = fetch(h, { { &n, h->kn_total.p, sizeof(int) } })) != LF_OK) return rc;
    *n_selected = n;
    return fetch(h, { { selected32, dsel, (size_t)n * 32 }, { query_idx, dqi, (size_t)n * 4 } });
}

extern "C" int lf_knn_match(lf_handle* h, const uint8_t* query32, int nq, const uint8_t* map32, int nm, int k, int32_t* idx, float* dist,
                            int on_device)
{
    if (!h) return LF_ERR_NOT_INITIALISED;
    if (nq < 0 || nm < 0 || k < 1 || k > 16 || (nq > 0 && (!query32 || !idx || !dist)) || (nm > 0 && !map32)) {
        lf_set_error(h, LF_ERR_BAD_ARG, "lf_knn_match: bad argument (k must be 1..16)");
        return LF_ERR_BAD_ARG;
    }
    if (nm > (1 << 24)) { lf_set_error(h, LF_ERR_UNSUPPORTED, "lf_knn_match: map larger than 2^24 entries"); return LF_ERR_UNSUPPORTED; }
    if (nq == 0) return LF_OK;
    LF_HIP_CHECK(h, hipSetDevice(h->device));
    hipStream_t s = h->stream;
    int rc;
    const size_t out = (size_t)nq * k;
    Staging st(h);
    const uint8_t* dq = st.in(on_device, query32, (size_t)nq * 32, h->a_q);
    const uint8_t* dm_ = st.in(on_device, map32, (size_t)nm * 32, h->a_m, 32);
    int32_t* didx = st.out(on_device, idx, out * 4, h->a_idx);
    float* ddist = st.out(on_device, dist, out * 4, h->a_dist);
    if ((rc = st.upload()) != LF_OK) return rc;
    { StageClock::Scope t(h, h->clock, ST_ASSOC); launch_knn(dq, nq, dm_, nm, k, 128, h->tie_rule == LF_TIE_MIHASHER, didx, ddist, s); }
    LF_HIP_CHECK(h, hipGetLastError());
    return fetch(h, { { idx, didx, out * 4 }, { dist, ddist, out * 4 } });
}

extern "C" int lf_radius_match(lf_handle* h, const uint8_t* query32, int nq, const uint8_t* map32, int nm, float max_distance,
                               int32_t* offsets, int32_t* idx, float* dist, int cap, int* total_out, int on_device)
{
    if (!h) return LF_ERR_NOT_INITIALISED;
    if (nq < 0 || nm < 0 || cap < 0 || !offsets || (cap > 0 && (!idx || !dist)) || (nq > 0 && !query32) || (nm > 0 && !map32) || !(max_distance >= 0)) {
        lf_set_error(h, LF_ERR_BAD_ARG, "lf_radius_match: bad argument");
        return LF_ERR_BAD_ARG;
    }
    if (nm > (1 << 24)) { lf_set_error(h, LF_ERR_UNSUPPORTED, "lf_radius_match: map larger than 2^24 entries"); return LF_ERR_UNSUPPORTED; }
    // K = N results are only ever collected up to D = 128 bits (Mihasher, :721), then filtered by maxDistance (:474)
    int md = max_distance >= 128.f ? 128 : (int)max_distance;
    LF_HIP_CHECK(h, hipSetDevice(h->device));
    hipStream_t s = h->stream;
    if (nq == 0) { if (on_device) LF_HIP_CHECK(h, hipMemsetAsync(offsets, 0, sizeof(int32_t), s)); else offsets[0] = 0; if (total_out) *total_out = 0; return LF_OK; }
    int rc;
    if ((rc = scratch(h, h->kn_hist, (size_t)nq * 129 * 4)) || (rc = scratch(h, h->kn_count, (size_t)nq * 4)) || (rc = scratch(h, h->kn_off, (size_t)(nq + 1) * 4)) ||
        (rc = scratch(h, h->kn_total, 16))) return rc;
    Staging st(h);
    const uint8_t* dq = st.in(on_device, query32, (size_t)nq * 32, h->a_q);
    const uint8_t* dm_ = st.in(on_device, map32, (size_t)nm * 32, h->a_m, 32);
    int32_t* doff = st.out(on_device, offsets, (size_t)(nq + 1) * 4, h->kn_off);
    int32_t* didx = st.out(on_device, idx, (size_t)(cap > 0 ? cap : 1) * 4, h->a_idx);
    float* ddist = st.out(on_device, dist, (size_t)(cap > 0 ? cap : 1) * 4, h->a_dist);
    if ((rc = st.upload()) != LF_OK) return rc;
    {
        StageClock::Scope t(h, h->clock, ST_ASSOC);
        launch_radius(dq, nq, dm_, nm, md, (int32_t*)h->kn_hist.p, (int32_t*)h->kn_count.p, doff, (int*)h->kn_total.p, cap, h->tie_rule == LF_TIE_MIHASHER, didx, ddist, s);
    }
    LF_HIP_CHECK(h, hipGetLastError());
    int total = 0;
    if ((rc = fetch(h, { { &total, h->kn_total.p, sizeof(int) }, { offsets, doff, (size_t)(nq + 1) * 4 } })) != LF_OK) return rc;
    if (total_out) *total_out = total;
    if (total > cap) { lf_set_error(h, LF_ERR_CAPACITY, "lf_radius_match: %d matches exceed the capacity %d (offsets are complete: size the arrays from them)", total, cap); return LF_ERR_CAPACITY; }
    return fetch(h, { { idx, didx, (size_t)total * 4 }, { dist, ddist, (size_t)total * 4 } });
}

// ---------------------------------------------------------------------------------------- the dataset form
static int matcher_image_of(const MatcherState* m, int row)
{
    // itup = indexesMap.upper_bound(row); itup--;  itup->second
    auto it = std::upper_bound(m->index_map.begin(), m->index_map.end(), std::make_pair(row, 0x7fffffff));
    return it == m->index_map.begin() ? 0 : (it - 1)->second;
}

extern "C" int lf_matcher_add(lf_handle* h, const uint8_t* codes32, int n, int on_device)
{
    if (!h) return LF_ERR_NOT_INITIALISED;
    if (n < 0 || (n > 0 && !codes32)) { lf_set_error(h, LF_ERR_BAD_ARG, "lf_matcher_add: bad argument"); return LF_ERR_BAD_ARG; }
    if (!h->matcher) { h->matcher.reset(new (std::nothrow) MatcherState()); if (!h->matcher) return LF_ERR_HIP; }
    MatcherState* m = h->matcher.get();
    if ((long long)m->total + n > (1 << 21)) { lf_set_error(h, LF_ERR_CAPACITY, "lf_matcher_add: the set would hold more than 2^21 descriptors"); return LF_ERR_CAPACITY; }
    LF_HIP_CHECK(h, hipSetDevice(h->device));
    if (n > 0) {
        const size_t need = (size_t)(m->total + n) * 32;
        if (need > m->codes.bytes) {                                       // grow, keeping what is there
            DevBuf grown;
            LF_HIP_CHECK(h, grown.alloc(need + need / 2 + 4096));
            if (m->total) LF_HIP_CHECK(h, hipMemcpyAsync(grown.p, m->codes.p, (size_t)m->total * 32, hipMemcpyDeviceToDevice, h->stream));
            LF_HIP_CHECK(h, hipStreamSynchronize(h->stream));
            m->codes = std::move(grown);
        }
        LF_HIP_CHECK(h, hipMemcpyAsync(static_cast<uint8_t*>(m->codes.p) + (size_t)m->total * 32, codes32, (size_t)n * 32,
                                       on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, h->stream));
        LF_HIP_CHECK(h, hipStreamSynchronize(h->stream));
    }
    // indexesMap.insert(pair(nextAddedIndex, numImages)): std::map::insert does NOT overwrite -- an image added right after an
    // EMPTY one finds the key taken and gets no entry of its own (its rows are reported under the empty image's number);
    // numImages still counts it
    if (m->index_map.empty() || m->index_map.back().first != m->total) m->index_map.push_back(std::make_pair(m->total, m->num_images));
    m->num_images += 1;
    m->total += n;
    return LF_OK;
}

extern "C" int lf_matcher_clear(lf_handle* h)
{
    if (!h) return LF_ERR_NOT_INITIALISED;
    if (h->matcher) { h->matcher->index_map.clear(); h->matcher->num_images = 0; h->matcher->total = 0; }
    return LF_OK;
}

extern "C" int lf_matcher_size(const lf_handle* h, int* n_images, int* n_descriptors)
{
    if (!h) return LF_ERR_NOT_INITIALISED;
    if (n_images) *n_images = h->matcher ? h->matcher->num_images : 0;
    if (n_descriptors) *n_descriptors = h->matcher ? h->matcher->total : 0;
    return LF_OK;
}

static int matcher_ready(lf_handle* h, const uint8_t* query32, int nq, const char* who)
{
    if (!h) return LF_ERR_NOT_INITIALISED;
    if (nq < 1 || !query32) { lf_set_error(h, LF_ERR_BAD_ARG, "%s: the query descriptors' matrix is empty", who); return LF_ERR_BAD_ARG; }
    if (!h->matcher || h->matcher->total < 1) { lf_set_error(h, LF_ERR_BAD_ARG, "%s: the dataset holds no descriptor (lf_matcher_add first)", who); return LF_ERR_BAD_ARG; }
    return LF_OK;
}

// The course of the three searches: the queries go up, `search` runs a pair form on the device -- the queries against the set, its
// lists into arrays of `room` entries, the offsets of a radius search into nq + 1 -- and leaves in *n how many entries it wrote;
// those come down into idx and dist, and the offsets into off where it is given.
typedef std::function<int(const uint8_t* dq, int32_t* doff, int32_t* didx, float* ddist, size_t* n)> MatcherSearch;

static int matcher_search(lf_handle* h, const uint8_t* query32, int nq, size_t room, std::vector<int32_t>* off, std::vector<int32_t>* idx,
                          std::vector<float>* dist, const MatcherSearch& search)
{
    MatcherState* m = h->matcher.get();
    int rc;
    Staging st(h);
    const uint8_t* dq = st.in(0, query32, (size_t)nq * 32, m->q);
    int32_t* doff = off ? st.out<int32_t>(0, nullptr, ((size_t)nq + 1) * 4, m->off) : nullptr;
    int32_t* didx = st.out<int32_t>(0, nullptr, room * 4, m->idx);
    float* ddist = st.out<float>(0, nullptr, room * 4, m->dist);
    if ((rc = st.upload()) != LF_OK) return rc;
    size_t n = room;
    if ((rc = search(dq, doff, didx, ddist, &n)) != LF_OK) return rc;
    if (off) off->resize((size_t)nq + 1);
    idx->resize(n); dist->resize(n);
    return fetch(h, { { off ? off->data() : nullptr, doff, ((size_t)nq + 1) * 4 }, { idx->data(), didx, n * 4 }, { dist->data(), ddist, n * 4 } });
}

extern "C" int lf_matcher_match(lf_handle* h, const uint8_t* query32, int nq, const uint8_t* const* masks, lf_dmatch* out, int* n_out)
{
    int rc = matcher_ready(h, query32, nq, "lf_matcher_match");
    if (rc != LF_OK) return rc;
    if (!out || !n_out) { lf_set_error(h, LF_ERR_BAD_ARG, "lf_matcher_match: null output"); return LF_ERR_BAD_ARG; }
    MatcherState* m = h->matcher.get();
    std::vector<int32_t> idx;
    std::vector<float> dist;
    rc = matcher_search(h, query32, nq, (size_t)nq, nullptr, &idx, &dist, [&](const uint8_t* dq, int32_t*, int32_t* didx, float* ddist, size_t*) {
        return lf_associate(h, dq, nq, static_cast<const uint8_t*>(m->codes.p), m->total, didx, ddist, 1);
    });
    if (rc != LF_OK) return rc;
    int n = 0;
    for (int qi = 0; qi < nq; ++qi) {
        if (idx[qi] < 0) continue;                                         // nothing within 128 bits: the reference's result is unset there
        const int img = matcher_image_of(m, idx[qi]);
        if (masks && masks[img] && masks[img][qi] == 0) continue;          // (:174: masks.empty() || masks[imgIdx].at<uchar>(counter) != 0)
        out[n].queryIdx = qi; out[n].trainIdx = idx[qi]; out[n].imgIdx = img; out[n].distance = dist[qi];
        ++n;
    }
    *n_out = n;
    return LF_OK;
}

extern "C" int lf_matcher_knn_match(lf_handle* h, const uint8_t* query32, int nq, int k, const uint8_t* const* masks, int compact_result,
                                    int32_t* list_offsets, lf_dmatch* out, int* n_lists)
{
    int rc = matcher_ready(h, query32, nq, "lf_matcher_knn_match");
    if (rc != LF_OK) return rc;
    if (!out || !n_lists || !list_offsets || k < 1 || k > 16) { lf_set_error(h, LF_ERR_BAD_ARG, "lf_matcher_knn_match: null output or k outside 1..16"); return LF_ERR_BAD_ARG; }
    MatcherState* m = h->matcher.get();
    const size_t nk = (size_t)nq * k;
    std::vector<int32_t> idx;
    std::vector<float> dist;
    rc = matcher_search(h, query32, nq, nk, nullptr, &idx, &dist, [&](const uint8_t* dq, int32_t*, int32_t* didx, float* ddist, size_t*) {
        return lf_knn_match(h, dq, nq, static_cast<const uint8_t*>(m->codes.p), m->total, k, didx, ddist, 1);
    });
    if (rc != LF_OK) return rc;
    int lists = 0, n = 0;
    list_offsets[0] = 0;
    for (int qi = 0; qi < nq; ++qi) {
        const int n0 = n;
        for (int j = 0; j < k; ++j) {
            const int32_t t = idx[(size_t)qi * k + j];
            if (t < 0) continue;
            const int img = matcher_image_of(m, t);
            if (masks && masks[img] && masks[img][qi] == 0) continue;
            out[n].queryIdx = qi; out[n].trainIdx = t; out[n].imgIdx = img; out[n].distance = dist[(size_t)qi * k + j];
            ++n;
        }
        // :417  (tempVector.size() == 0 && !compactResult) || tempVector.size() > 0
        if (n > n0 || !compact_result) list_offsets[++lists] = n;
    }
    *n_lists = lists;
    return LF_OK;
}

extern "C" int lf_matcher_radius_match(lf_handle* h, const uint8_t* query32, int nq, float max_distance, const uint8_t* const* masks,
                                       int compact_result, int32_t* list_offsets, lf_dmatch* out, int cap, int* n_lists, int* total)
{
    int rc = matcher_ready(h, query32, nq, "lf_matcher_radius_match");
    if (rc != LF_OK) return rc;
    if (!n_lists || !list_offsets || !total || cap < 0 || (cap > 0 && !out)) { lf_set_error(h, LF_ERR_BAD_ARG, "lf_matcher_radius_match: bad argument"); return LF_ERR_BAD_ARG; }
    MatcherState* m = h->matcher.get();
    std::vector<int32_t> off, idx;
    std::vector<float> dist;
    rc = matcher_search(h, query32, nq, (size_t)(cap > 0 ? cap : 1), &off, &idx, &dist, [&](const uint8_t* dq, int32_t* doff, int32_t* didx, float* ddist, size_t* n) {
        int found = 0;
        const int rc_search = lf_radius_match(h, dq, nq, static_cast<const uint8_t*>(m->codes.p), m->total, max_distance, doff, didx, ddist, cap, &found, 1);
        *total = found;                                                    // (before the masks: the capacity the search itself needs)
        *n = (size_t)found;
        return rc_search;
    });
    if (rc != LF_OK) return rc;
    int lists = 0, n = 0;
    list_offsets[0] = 0;
    for (int qi = 0; qi < nq; ++qi) {
        const int n0 = n;
        for (int j = off[qi]; j < off[qi + 1]; ++j) {
            const int img = matcher_image_of(m, idx[j]);
            if (masks && masks[img] && masks[img][qi] == 0) continue;
            out[n].queryIdx = qi; out[n].trainIdx = idx[j]; out[n].imgIdx = img; out[n].distance = dist[j];
            ++n;
        }
        if (n > n0 || !compact_result) list_offsets[++lists] = n;
    }
    *n_lists = lists;
    return LF_OK;
}
