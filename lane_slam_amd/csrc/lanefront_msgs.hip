// lanefront C ABI, the SegmentList glue: a batch's segments to and from the bodies of duckietown_msgs/SegmentList messages
// (k_msgs.hip), with the segments and the bodies each on the host or on the device.
#include "lanefront_handle.h"

using namespace lf;

extern "C" int lf_serialize_segments(lf_handle* h, const lf_segments* segs, int segs_on_device, int n_frames, int stage,
                                     uint8_t* out, size_t out_capacity, int out_on_device, int64_t* frame_byte_offset)
{
    if (!h) return LF_ERR_NOT_INITIALISED;
    if (!segs || !out || !frame_byte_offset || n_frames < 1 || stage < LF_MSG_DETECTOR || stage > LF_MSG_FILTERED || !segs->frame_offset || !segs->color) {
        lf_set_error(h, LF_ERR_BAD_ARG, "lf_serialize_segments: null argument, n_frames < 1 or unknown stage");
        return LF_ERR_BAD_ARG;
    }
    if (stage == LF_MSG_DETECTOR ? (!segs->pixels_normalized || !segs->normals) : (!segs->ground || (stage == LF_MSG_FILTERED && !segs->keep))) {
        lf_set_error(h, LF_ERR_BAD_ARG, "lf_serialize_segments: the arrays of stage %d are missing", stage);
        return LF_ERR_BAD_ARG;
    }
    LF_HIP_CHECK(h, hipSetDevice(h->device));
    hipStream_t s = h->stream;
    int rc;
    // (only the arrays of the stage travel, each with the caller's own total of segments)
    size_t n = 0;
    if (!segs_on_device) {
        const int total = segs->frame_offset[n_frames];
        if (total < 0) { lf_set_error(h, LF_ERR_BAD_ARG, "negative segment count"); return LF_ERR_BAD_ARG; }
        n = (size_t)total;
    }
    const bool det = stage == LF_MSG_DETECTOR, filtered = stage == LF_MSG_FILTERED;
    Staging st(h);
    const int* d_fo = st.in(segs_on_device, segs->frame_offset, (size_t)(n_frames + 1) * sizeof(int), h->m_fo);
    const uint8_t* d_color = st.in(segs_on_device, segs->color, n, h->m_color, n + 1);
    const float* d_pn = det ? st.in(segs_on_device, segs->pixels_normalized, n * 16, h->m_pn, n * 16 + 16) : segs->pixels_normalized;
    const float* d_nm = det ? st.in(segs_on_device, segs->normals, n * 8, h->m_nm, n * 8 + 8) : segs->normals;
    const double* d_gr = det ? segs->ground : st.in(segs_on_device, segs->ground, n * 32, h->m_gr, n * 32 + 32);
    const uint8_t* d_keep = filtered ? st.in(segs_on_device, segs->keep, n, h->m_keep, n + 1) : segs->keep;
    if ((rc = scratch(h, h->m_counts, (size_t)n_frames * sizeof(int))) || (rc = scratch(h, h->m_boff, (size_t)(n_frames + 1) * sizeof(long long)))) return rc;
    if ((rc = st.upload()) != LF_OK) return rc;
    launch_msg_layout(n_frames, stage, d_fo, d_keep, static_cast<int*>(h->m_counts.p), static_cast<long long*>(h->m_boff.p), s);
    static_assert(sizeof(long long) == sizeof(int64_t), "byte offsets are int64");
    if ((rc = fetch(h, { { frame_byte_offset, h->m_boff.p, (size_t)(n_frames + 1) * sizeof(long long) } })) != LF_OK) return rc;
    const size_t need = (size_t)frame_byte_offset[n_frames];
    if (need > out_capacity) {
        lf_set_error(h, LF_ERR_CAPACITY, "lf_serialize_segments: %zu bytes needed, %zu available", need, out_capacity);
        return LF_ERR_CAPACITY;
    }
    uint8_t* d_out = st.out(out_on_device, out, need + 16, h->m_body);
    if ((rc = st.upload()) != LF_OK) return rc;              // (the growth's result: nothing is left to copy)
    launch_msg_write(n_frames, stage, d_fo, d_color, d_pn, d_nm, d_gr, d_keep, static_cast<const int*>(h->m_counts.p),
                     static_cast<const long long*>(h->m_boff.p), d_out, s);
    LF_HIP_CHECK(h, hipGetLastError());
    return fetch(h, { { out, d_out, need } });
}

extern "C" int lf_deserialize_segments(lf_handle* h, const uint8_t* bodies, int bodies_on_device, const int64_t* frame_byte_offset,
                                       int n_frames, lf_segments* out, int out_on_device, int* n_segments)
{
    if (!h) return LF_ERR_NOT_INITIALISED;
    if (!bodies || !frame_byte_offset || !out || n_frames < 1 || !out->frame_offset) {
        lf_set_error(h, LF_ERR_BAD_ARG, "lf_deserialize_segments: null argument or n_frames < 1");
        return LF_ERR_BAD_ARG;
    }
    for (int f = 0; f < n_frames; ++f)
        if (frame_byte_offset[f + 1] < frame_byte_offset[f] + 4) { lf_set_error(h, LF_ERR_DECODE, "body %d is shorter than its count field", f); return LF_ERR_DECODE; }
    LF_HIP_CHECK(h, hipSetDevice(h->device));
    hipStream_t s = h->stream;
    const size_t bytes = (size_t)frame_byte_offset[n_frames];
    const size_t max_segs = bytes / 73 + 1;
    int rc;
    Staging st(h);
    const uint8_t* d_body = st.in(bodies_on_device, bodies, bytes, h->m_body, bytes + 16);
    const long long* d_boff = st.in(0, reinterpret_cast<const long long*>(frame_byte_offset), (size_t)(n_frames + 1) * sizeof(long long), h->m_boff);
    if ((rc = scratch(h, h->m_bad, sizeof(int))) != LF_OK) return rc;
    // (an array the caller did not ask for stays null: the kernel leaves it out)
    lf_segments dev = *out;
    dev.frame_offset = st.out(out_on_device, out->frame_offset, (size_t)(n_frames + 1) * sizeof(int), h->m_fo);
    if (out->color) dev.color = st.out(out_on_device, out->color, max_segs, h->m_color);
    if (out->pixels_normalized) dev.pixels_normalized = st.out(out_on_device, out->pixels_normalized, max_segs * 16, h->m_pn);
    if (out->normals) dev.normals = st.out(out_on_device, out->normals, max_segs * 8, h->m_nm);
    if (out->ground) dev.ground = st.out(out_on_device, out->ground, max_segs * 32, h->m_gr);
    if ((rc = st.upload()) != LF_OK) return rc;
    LF_HIP_CHECK(h, hipMemsetAsync(h->m_bad.p, 0, sizeof(int), s));
    const int cap = out->capacity;
    launch_msg_read(n_frames, cap, d_body, d_boff, dev.frame_offset, static_cast<int*>(h->m_bad.p),
                    dev.color, dev.pixels_normalized, dev.normals, dev.ground, s);
    LF_HIP_CHECK(h, hipGetLastError());
    int bad = 0, total = 0;
    if ((rc = fetch(h, { { &bad, h->m_bad.p, sizeof(int) }, { &total, dev.frame_offset + n_frames, sizeof(int) } })) != LF_OK) return rc;
    if (n_segments) *n_segments = total;
    if (bad) { lf_set_error(h, LF_ERR_DECODE, "a SegmentList body's count does not match its length"); return LF_ERR_DECODE; }
    if (total > cap) { lf_set_error(h, LF_ERR_CAPACITY, "%d segments exceed the output capacity %d", total, cap); return LF_ERR_CAPACITY; }
    const size_t n = (size_t)total;
    return fetch(h, { { out->frame_offset, dev.frame_offset, (size_t)(n_frames + 1) * sizeof(int) }, { out->color, dev.color, n },
                      { out->pixels_normalized, dev.pixels_normalized, n * 16 }, { out->normals, dev.normals, n * 8 }, { out->ground, dev.ground, n * 32 } });
}
