// The baseline JPEG encoder of jpg_from_image_cv (k_jenc.hip): what libjpeg writes for cv2.imencode('.jpg', bgr) -- YCbCr 4:2:0, the
// integer "islow" DCT, the annex K Huffman tables, one scan.  tests/jpeg_enc_ref.py is the same arithmetic in numpy and says where
// each stage comes from.  Shared by the kernels and the host side (lanefront_jenc.hip): the geometry, the buffer sizes and the
// per-call tables.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <hip/hip_runtime.h>

namespace lf {
namespace jenc {

constexpr int kHeaderMax = 640;              // SOI .. SOS is 623 bytes
// A block's bits never exceed a DC symbol (11 + 11) and 63 AC symbols of 16 + 10 bits: 1660 bits; the buffers take 208 bytes.
constexpr int kBlockBytesMax = 208;
constexpr int kChunkBytes = 4096;            // bytes of the unstuffed scan one workgroup of the stuffing pass handles (256 x 16)
constexpr int kStages = 8;                   // transform, size, scan, zero, emit, count, scan, write

struct Geom {
    int rows, cols, mr, mc;                  // the image, and its 16 x 16 MCUs
    int blocks;                              // mr * mc * 6, scan order: per MCU Y00 Y01 Y10 Y11 Cb Cr
    int words;                               // 32-bit words of one frame's unstuffed bit buffer (a multiple of 4): blocks * 52
    int chunks;                              // ceil(words * 4 / kChunkBytes)
};
inline Geom geom(int rows, int cols)
{
    Geom g;
    g.rows = rows; g.cols = cols; g.mr = (rows + 15) / 16; g.mc = (cols + 15) / 16;
    g.blocks = g.mr * g.mc * 6;
    g.words = g.blocks * (kBlockBytesMax / 4);
    g.chunks = (int)(((size_t)g.words * 4 + kChunkBytes - 1) / kChunkBytes);
    return g;
}

// What a call's kernels read besides the image: built on the host for (rows, cols, quality), copied when one of them changes
struct Tables {
    uint16_t div[2][64];                     // quantisation divisors (q << 3) in ZIGZAG order: luma, chroma
    uint32_t dc[2][16];                      // code | length << 16 per DC category
    uint32_t ac[2][256];                     // code | length << 16 per run / size symbol (0x00 EOB, 0xF0 ZRL)
    int32_t header_len;
    uint8_t header[kHeaderMax];
};

// every block of n frames: coef int16 [n][blocks][64] zigzag (a dummy block's are zero)
void launch_transform(const uint8_t* bgr, int n, const Geom& g, const Tables* tab, int16_t* coef, hipStream_t s);
// bits [n][blocks]: each block's length in bits; dcdiff [n][blocks]: its DC difference
void launch_size(const int16_t* coef, int n, const Geom& g, const Tables* tab, uint32_t* bits, int16_t* dcdiff, hipStream_t s);
// bits -> its exclusive scan per frame, in place; total_bits [n]
void launch_scan_bits(uint32_t* bits, int n, const Geom& g, uint32_t* total_bits, hipStream_t s);
// zero the words of every frame's bit buffer [n][words] that its scan reaches
void launch_zero(const uint32_t* total_bits, int n, const Geom& g, uint32_t* bitbuf, hipStream_t s);
// every block's bits at its offset
void launch_emit(const int16_t* coef, const int16_t* dcdiff, const uint32_t* bit_off, const uint32_t* total_bits, int n, const Geom& g,
                 const Tables* tab, uint32_t* bitbuf, hipStream_t s);
// the stuffing pass: ff [n][chunks] = 0xFF bytes per chunk of the padded scan; then its exclusive scan and out_size [n], the file's
// bytes or 0 when it does not fit out_stride; then header, stuffed scan and EOI of every frame that fits
void launch_ff_count(const uint32_t* bitbuf, const uint32_t* total_bits, int n, const Geom& g, uint32_t* ff, hipStream_t s);
void launch_ff_scan(const uint32_t* total_bits, int n, const Geom& g, const Tables* tab, uint32_t* ff, size_t out_stride, uint32_t* out_size,
                    hipStream_t s);
void launch_write(const uint32_t* bitbuf, const uint32_t* total_bits, const uint32_t* ff, const uint32_t* out_size, int n, const Geom& g,
                  const Tables* tab, uint8_t* out, size_t out_stride, hipStream_t s);

}  // namespace jenc
}  // namespace lf
