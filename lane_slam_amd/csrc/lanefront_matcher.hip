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

#include <string.h>
#include <algorithm>
#include "lanefront_handle.h"

using namespace lf;

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

extern "C" int lf_matcher_match(lf_handle* h, const uint8_t* query32, int nq, const uint8_t* const* masks, lf_dmatch* out, int* n_out)
{
    int rc = matcher_ready(h, query32, nq, "lf_matcher_match");
    if (rc != LF_OK) return rc;
    if (!out || !n_out) { lf_set_error(h, LF_ERR_BAD_ARG, "lf_matcher_match: null output"); return LF_ERR_BAD_ARG; }
    MatcherState* m = h->matcher.get();
    std::vector<int32_t> idx((size_t)nq);
    std::vector<float> dist((size_t)nq);
    if ((rc = scratch(h, m->q, (size_t)nq * 32)) || (rc = scratch(h, m->idx, (size_t)nq * 4)) || (rc = scratch(h, m->dist, (size_t)nq * 4))) return rc;
    LF_HIP_CHECK(h, hipMemcpyAsync(m->q.p, query32, (size_t)nq * 32, hipMemcpyHostToDevice, h->stream));
    if ((rc = lf_associate(h, static_cast<const uint8_t*>(m->q.p), nq, static_cast<const uint8_t*>(m->codes.p), m->total,
                           static_cast<int32_t*>(m->idx.p), static_cast<float*>(m->dist.p), 1)) != LF_OK) return rc;
    LF_HIP_CHECK(h, hipMemcpyAsync(idx.data(), m->idx.p, (size_t)nq * 4, hipMemcpyDeviceToHost, h->stream));
    LF_HIP_CHECK(h, hipMemcpyAsync(dist.data(), m->dist.p, (size_t)nq * 4, hipMemcpyDeviceToHost, h->stream));
    LF_HIP_CHECK(h, hipStreamSynchronize(h->stream));
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
    std::vector<int32_t> idx(nk);
    std::vector<float> dist(nk);
    if ((rc = scratch(h, m->q, (size_t)nq * 32)) || (rc = scratch(h, m->idx, nk * 4)) || (rc = scratch(h, m->dist, nk * 4))) return rc;
    LF_HIP_CHECK(h, hipMemcpyAsync(m->q.p, query32, (size_t)nq * 32, hipMemcpyHostToDevice, h->stream));
    if ((rc = lf_knn_match(h, static_cast<const uint8_t*>(m->q.p), nq, static_cast<const uint8_t*>(m->codes.p), m->total, k,
                           static_cast<int32_t*>(m->idx.p), static_cast<float*>(m->dist.p), 1)) != LF_OK) return rc;
    LF_HIP_CHECK(h, hipMemcpyAsync(idx.data(), m->idx.p, nk * 4, hipMemcpyDeviceToHost, h->stream));
    LF_HIP_CHECK(h, hipMemcpyAsync(dist.data(), m->dist.p, nk * 4, hipMemcpyDeviceToHost, h->stream));
    LF_HIP_CHECK(h, hipStreamSynchronize(h->stream));
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
    if ((rc = scratch(h, m->q, (size_t)nq * 32)) || (rc = scratch(h, m->off, ((size_t)nq + 1) * 4)) ||
        (rc = scratch(h, m->idx, (size_t)(cap > 0 ? cap : 1) * 4)) || (rc = scratch(h, m->dist, (size_t)(cap > 0 ? cap : 1) * 4))) return rc;
    LF_HIP_CHECK(h, hipMemcpyAsync(m->q.p, query32, (size_t)nq * 32, hipMemcpyHostToDevice, h->stream));
    int found = 0;
    rc = lf_radius_match(h, static_cast<const uint8_t*>(m->q.p), nq, static_cast<const uint8_t*>(m->codes.p), m->total, max_distance,
                         static_cast<int32_t*>(m->off.p), static_cast<int32_t*>(m->idx.p), static_cast<float*>(m->dist.p), cap, &found, 1);
    *total = found;                                                        // (before the masks: the capacity the search itself needs)
    if (rc != LF_OK) return rc;
    std::vector<int32_t> off((size_t)nq + 1), idx((size_t)found);
    std::vector<float> dist((size_t)found);
    LF_HIP_CHECK(h, hipMemcpyAsync(off.data(), m->off.p, ((size_t)nq + 1) * 4, hipMemcpyDeviceToHost, h->stream));
    if (found) {
        LF_HIP_CHECK(h, hipMemcpyAsync(idx.data(), m->idx.p, (size_t)found * 4, hipMemcpyDeviceToHost, h->stream));
        LF_HIP_CHECK(h, hipMemcpyAsync(dist.data(), m->dist.p, (size_t)found * 4, hipMemcpyDeviceToHost, h->stream));
    }
    LF_HIP_CHECK(h, hipStreamSynchronize(h->stream));
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
