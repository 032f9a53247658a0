// Host side of the JPEG encoder (k_jenc.hip): the per-call tables and header, the buffers, the launches, the delivery.
#include <string.h>
#include <initializer_list>
#include "lanefront_handle.h"
#include "k_jenc.h"

using namespace lf;

namespace {

constexpr int kMaxSide = 8192;        // a frame's bit offsets stay within 32 bits and its word count within an int
constexpr int kMaxFrames = 65535;     // a grid dimension

const uint8_t kZigzag[64] = { 0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                              35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63 };
// ITU-T T.81 annex K.1: the luminance and chrominance quantisation tables, natural order
const uint8_t kStdQ[2][64] = {
    { 16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,  69,  56,  14, 17, 22, 29, 51,  87,  80,  62,
      18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,  49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99 },
    { 17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
      99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99 } };
// annex K.3: codes per length 1 .. 16, then the symbols in code order
const uint8_t kDcBits[2][16] = { { 0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0 }, { 0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0 } };
const uint8_t kDcVals[12] = { 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11 };
const uint8_t kAcBits[2][16] = { { 0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d }, { 0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77 } };
const uint8_t kAcVals[2][162] = {
    { 0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
      0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
      0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
      0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
      0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
      0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
      0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
      0xfa },
    { 0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
      0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
      0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
      0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
      0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
      0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
      0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
      0xfa } };

// jchuff.c jpeg_make_c_derived_tbl: code | length << 16 per symbol
void derive(const uint8_t* bits, const uint8_t* vals, uint32_t* out, int n_out)
{
    for (int k = 0; k < n_out; ++k) out[k] = 0;
    uint32_t code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int i = 0; i < bits[len - 1]; ++i, ++k, ++code)
            if (vals[k] < n_out) out[vals[k]] = code | (uint32_t)len << 16;
        code <<= 1;
    }
}

// jpeg_set_quality(quality, TRUE)'s tables, then everything jcmarker.c writes before the scan
void make_tables(int rows, int cols, int quality, jenc::Tables* t)
{
    memset(t, 0, sizeof(*t));
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    uint8_t q[2][64];
    for (int c = 0; c < 2; ++c)
        for (int k = 0; k < 64; ++k) {
            int v = (kStdQ[c][k] * scale + 50) / 100;
            v = v < 1 ? 1 : v > 255 ? 255 : v;
            q[c][k] = (uint8_t)v;
        }
    for (int c = 0; c < 2; ++c) {
        for (int k = 0; k < 64; ++k) t->div[c][k] = (uint16_t)(q[c][kZigzag[k]] << 3);
        derive(kDcBits[c], kDcVals, t->dc[c], 16);
        derive(kAcBits[c], kAcVals[c], t->ac[c], 256);
    }
    uint8_t* p = t->header;
    auto put = [&p](std::initializer_list<int> v) { for (int b : v) *p++ = (uint8_t)b; };
    put({ 0xFF, 0xD8, 0xFF, 0xE0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0 });
    for (int c = 0; c < 2; ++c) {
        put({ 0xFF, 0xDB, 0, 67, c });
        for (int k = 0; k < 64; ++k) *p++ = q[c][kZigzag[k]];
    }
    put({ 0xFF, 0xC0, 0, 17, 8, rows >> 8, rows & 255, cols >> 8, cols & 255, 3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1 });
    for (int c = 0; c < 2; ++c)
        for (int ac = 0; ac < 2; ++ac) {
            const uint8_t* bits = ac ? kAcBits[c] : kDcBits[c];
            const uint8_t* vals = ac ? kAcVals[c] : kDcVals;
            const int n = ac ? 162 : 12;
            put({ 0xFF, 0xC4, (19 + n) >> 8, (19 + n) & 255, ac << 4 | c });
            for (int k = 0; k < 16; ++k) *p++ = bits[k];
            for (int k = 0; k < n; ++k) *p++ = vals[k];
        }
    put({ 0xFF, 0xDA, 0, 12, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0 });
    t->header_len = (int32_t)(p - t->header);
}

size_t header_bytes()
{
    static const size_t n = [] { jenc::Tables t; make_tables(1, 1, 95, &t); return (size_t)t.header_len; }();
    return n;
}

bool size_ok(int rows, int cols) { return rows >= 1 && cols >= 1 && rows <= kMaxSide && cols <= kMaxSide; }

}  // namespace

extern "C" size_t lf_jpeg_encode_bound(int rows, int cols)
{
    if (!size_ok(rows, cols)) return 0;
    // every byte of the scan may be 0xFF and take a stuffed zero behind it; + EOI
    return header_bytes() + 2 * (size_t)jenc::geom(rows, cols).blocks * jenc::kBlockBytesMax + 2;
}

extern "C" int lf_jpeg_encode_batch(lf_handle* h, const uint8_t* bgr, int bgr_on_device, int n_frames, int rows, int cols, int quality, uint8_t* out,
                                    size_t out_stride, uint32_t* out_size, int out_on_device)
{
    if (!h) return LF_ERR_NOT_INITIALISED;
    if (!bgr || !out || !out_size) { lf_set_error(h, LF_ERR_BAD_ARG, "lf_jpeg_encode_batch: null argument"); return LF_ERR_BAD_ARG; }
    if (n_frames < 1 || n_frames > kMaxFrames) {
        lf_set_error(h, LF_ERR_BAD_ARG, "lf_jpeg_encode_batch: n_frames %d (1 .. %d)", n_frames, kMaxFrames);
        return LF_ERR_BAD_ARG;
    }
    if (!size_ok(rows, cols)) {
        lf_set_error(h, LF_ERR_BAD_ARG, "lf_jpeg_encode_batch: frames of %d x %d (1 .. %d px a side)", rows, cols, kMaxSide);
        return LF_ERR_BAD_ARG;
    }
    if (quality == 0) quality = 95;
    if (quality < 1 || quality > 100) {
        lf_set_error(h, LF_ERR_BAD_ARG, "lf_jpeg_encode_batch: quality %d (1 .. 100, 0 for cv2.imencode's 95)", quality);
        return LF_ERR_BAD_ARG;
    }
    if (out_stride < 1) { lf_set_error(h, LF_ERR_BAD_ARG, "lf_jpeg_encode_batch: out_stride 0"); return LF_ERR_BAD_ARG; }
    LF_HIP_CHECK(h, hipSetDevice(h->device));
    if (!h->jenc) h->jenc.reset(new JencState());
    JencState& e = *h->jenc;
    hipStream_t s = h->stream;
    const jenc::Geom g = jenc::geom(rows, cols);
    const size_t n = (size_t)n_frames, nb = n * g.blocks;
    int rc;
    // a host caller's slots are staged no wider than a frame can get
    const size_t bound = lf_jpeg_encode_bound(rows, cols), stage_stride = out_stride < bound ? out_stride : bound;
    if ((rc = scratch(h, e.tab, sizeof(jenc::Tables))) || (rc = scratch(h, e.coef, nb * 64 * sizeof(int16_t))) ||
        (rc = scratch(h, e.bits, nb * sizeof(uint32_t))) || (rc = scratch(h, e.dcdiff, nb * sizeof(int16_t))) ||
        (rc = scratch(h, e.total, n * sizeof(uint32_t))) || (rc = scratch(h, e.bitbuf, n * g.words * sizeof(uint32_t))) ||
        (rc = scratch(h, e.ff, n * g.chunks * sizeof(uint32_t))))
        return rc;
    Staging st(h);
    const uint8_t* src = st.in(bgr_on_device, bgr, n * rows * cols * 3, e.in);
    uint8_t* dst = st.out(out_on_device, out, n * stage_stride, e.out);
    uint32_t* dsz = st.out(out_on_device, out_size, n * sizeof(uint32_t), e.sizes);
    if (!e.h_tab.p) LF_HIP_CHECK(h, e.h_tab.alloc(sizeof(jenc::Tables)));
    if (!out_on_device && e.h_sizes.bytes < n * sizeof(uint32_t)) LF_HIP_CHECK(h, e.h_sizes.alloc(n * sizeof(uint32_t)));
    if (e.rows != rows || e.cols != cols || e.quality != quality) {
        // (the pinned copy may still be on its way to the device for a call before this one)
        if (e.quality) LF_HIP_CHECK(h, hipStreamSynchronize(s));
        make_tables(rows, cols, quality, e.h_tab.p);
        LF_HIP_CHECK(h, hipMemcpyAsync(e.tab.p, e.h_tab.p, sizeof(jenc::Tables), hipMemcpyHostToDevice, s));
        e.rows = rows; e.cols = cols; e.quality = quality;
    }
    if ((rc = st.upload()) != LF_OK) return rc;
    const size_t dstride = out_on_device ? out_stride : stage_stride;
    const jenc::Tables* tab = static_cast<const jenc::Tables*>(e.tab.p);
    int16_t* coef = static_cast<int16_t*>(e.coef.p);
    uint32_t* bits = static_cast<uint32_t*>(e.bits.p);
    int16_t* dcdiff = static_cast<int16_t*>(e.dcdiff.p);
    uint32_t* total = static_cast<uint32_t*>(e.total.p);
    uint32_t* bitbuf = static_cast<uint32_t*>(e.bitbuf.p);
    uint32_t* ff = static_cast<uint32_t*>(e.ff.p);
    if ((rc = e.clock.begin(h)) != LF_OK) return rc;
    { CallClock::Scope t(e.clock, 0); jenc::launch_transform(src, n_frames, g, tab, coef, s); }
    { CallClock::Scope t(e.clock, 1); jenc::launch_size(coef, n_frames, g, tab, bits, dcdiff, s); }
    { CallClock::Scope t(e.clock, 2); jenc::launch_scan_bits(bits, n_frames, g, total, s); }
    { CallClock::Scope t(e.clock, 3); jenc::launch_zero(total, n_frames, g, bitbuf, s); }
    { CallClock::Scope t(e.clock, 4); jenc::launch_emit(coef, dcdiff, bits, total, n_frames, g, tab, bitbuf, s); }
    { CallClock::Scope t(e.clock, 5); jenc::launch_ff_count(bitbuf, total, n_frames, g, ff, s); }
    { CallClock::Scope t(e.clock, 6); jenc::launch_ff_scan(total, n_frames, g, tab, ff, out_stride, dsz, s); }
    { CallClock::Scope t(e.clock, 7); jenc::launch_write(bitbuf, total, ff, dsz, n_frames, g, tab, dst, dstride, s); }
    LF_HIP_CHECK(h, hipGetLastError());
    if (out_on_device) return LF_OK;
    LF_HIP_CHECK(h, hipMemcpyAsync(e.h_sizes.p, dsz, n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    LF_HIP_CHECK(h, hipStreamSynchronize(s));
    int missing = 0;
    for (size_t f = 0; f < n; ++f) {
        out_size[f] = e.h_sizes.p[f];
        if (out_size[f] == 0) { ++missing; continue; }
        LF_HIP_CHECK(h, hipMemcpyAsync(out + f * out_stride, dst + f * dstride, out_size[f], hipMemcpyDeviceToHost, s));
    }
    LF_HIP_CHECK(h, hipStreamSynchronize(s));
    if (missing) {
        lf_set_error(h, LF_ERR_CAPACITY, "lf_jpeg_encode_batch: %d of %d frames need more than out_stride = %zu bytes (lf_jpeg_encode_bound: %zu)",
                     missing, n_frames, out_stride, bound);
        return LF_ERR_CAPACITY;
    }
    return LF_OK;
}

extern "C" int lf_jpeg_encode_timing(lf_handle* h, double* ms_per_stage, int n)
{
    if (!h) return LF_ERR_NOT_INITIALISED;
    if (!ms_per_stage || n < jenc::kStages) { lf_set_error(h, LF_ERR_BAD_ARG, "lf_jpeg_encode_timing: room for %d stages", jenc::kStages); return LF_ERR_BAD_ARG; }
    if (!h->jenc || !h->jenc->clock.timed) {
        lf_set_error(h, LF_ERR_BAD_ARG, "lf_jpeg_encode_timing: no lf_jpeg_encode_batch ran with profiling on (lf_set_profiling)");
        return LF_ERR_BAD_ARG;
    }
    return h->jenc->clock.read(h, jenc::kStages, ms_per_stage);
}

extern "C" const char* lf_jpeg_encode_stage_name(int stage)
{
    static const char* const names[jenc::kStages] = { "k_je_transform", "k_je_size", "k_je_scan_bits", "k_je_zero", "k_je_emit", "k_je_ff_count",
                                                      "k_je_ff_scan", "k_je_write" };
    return stage >= 0 && stage < jenc::kStages ? names[stage] : "";
}
